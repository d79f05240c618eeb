"""GPU tests of alternating unimodal training on a shared head (MLA; csrc/mla.hip, gdl.MLATrainer): the four gdl_mla_* launches
against the float64 restatement within its derived bounds (tests/mla_ref.py), the bit-level contracts (a symmetric projector,
in-place projection, identical bytes from two runs), and the runner against the torch float32 goldens
(tests/golden/make_golden_mla.py), against UnimodalTrainer, across a checkpoint, and its refusals."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fixtures as fx

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mla_ref as mref  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np(t):
    return t.detach().cpu().numpy()


def _feat(seed, B):
    gen = torch.Generator(device=DEV).manual_seed(7000 + seed)
    return torch.randn(B, 512, generator=gen, device=DEV).clamp_min(0)


def _within(got, want, bound, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    worst = float((err / bound).max())
    print(what, "worst share of the bound", worst)
    assert worst <= 1.0, (what, worst)


# ------------------------------------------------------------------ gdl_mla_feature_mean
def _mean(h):
    r = torch.full((512,), NAN, device=DEV)
    L.call("gdl_mla_feature_mean", L.ptr(h), h.shape[0], L.ptr(r), L.cur_stream())
    return r


@pytest.mark.parametrize("B", [1, 5, 64, 65, 257])
def test_feature_mean(B):
    h = _feat(B, B)
    r = _mean(h)
    _within(_np(r), mref.feature_mean(_np(h)), mref.feature_mean_bound(_np(h)), f"feature_mean B={B}")
    assert _same(r, _mean(h))


# ------------------------------------------------------------------ gdl_mla_projector_update
def _update(P, r, alpha, normalize):
    ws = torch.empty(L.load().gdl_mla_projector_workspace_bytes(), dtype=torch.uint8, device=DEV)
    L.call("gdl_mla_projector_update", L.ptr(P), L.ptr(r), float(alpha), int(normalize), L.ptr(ws), ws.numel(), L.cur_stream())
    return P


_P3 = {}


def _p_after_three():
    """A P that three earlier updates produced (made once, handed out as clones), each checked for exact symmetry."""
    if "P" not in _P3:
        P = torch.eye(512, device=DEV)
        for i in range(3):
            _update(P, _feat(100 + i, 64).mean(dim=0), 0.1, True)
            assert _same(P, P.t())
        _P3["P"] = P
    return _P3["P"].clone()


@pytest.mark.parametrize("rkind", ["features", "zero"])
@pytest.mark.parametrize("alpha", [0.1, 1e-3])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("start", ["identity", "three"])
def test_projector_update(start, normalize, alpha, rkind):
    P0 = torch.eye(512, device=DEV) if start == "identity" else _p_after_three()
    r = _feat(200, 64).mean(dim=0) if rkind == "features" else torch.zeros(512, device=DEV)
    P = _update(P0.clone(), r, alpha, normalize)
    res = mref.projector_update(_np(P0), _np(r), alpha, bool(normalize))
    _within(_np(P), res["P"], mref.projector_bounds(res)["P"], f"projector {start} normalize={normalize} alpha={alpha} {rkind}")
    assert _same(P, P.t()), "P must stay bit-identical to its transpose"
    assert _same(P, _update(P0.clone(), r, alpha, normalize)), "two runs give identical bytes"
    if rkind == "zero" and not normalize:
        assert _same(P, P0)
    if normalize:
        assert abs(float(P.double().pow(2).sum().sqrt()) - 1.0) < 1e-5


def test_projector_update_refusals():
    P, r = torch.eye(512, device=DEV), torch.zeros(512, device=DEV)
    ws = torch.empty(L.load().gdl_mla_projector_workspace_bytes(), dtype=torch.uint8, device=DEV)
    for alpha in (0.0, -1.0, float("inf"), NAN):
        with pytest.raises(L.GdlError):
            L.call("gdl_mla_projector_update", L.ptr(P), L.ptr(r), alpha, 1, L.ptr(ws), ws.numel(), L.cur_stream())
    with pytest.raises(L.GdlError):
        L.call("gdl_mla_projector_update", L.ptr(P), L.ptr(r), 0.1, 1, L.ptr(ws), ws.numel() - 4, L.cur_stream())
    torch.cuda.synchronize()
    assert _same(P, torch.eye(512, device=DEV))


# ------------------------------------------------------------------ gdl_mla_project
@pytest.mark.parametrize("n", [6, 34, 309, 512])
def test_project(n):
    gen = torch.Generator(device=DEV).manual_seed(300 + n)
    P = _p_after_three() + 0.01 * torch.randn(512, 512, generator=gen, device=DEV)  # not symmetric: P^T is not P
    dW0 = torch.randn(n, 512, generator=gen, device=DEV) / 64
    dW = dW0.clone()
    L.call("gdl_mla_project", L.ptr(dW), L.ptr(P), n, L.cur_stream())
    _within(_np(dW), mref.project(_np(dW0), _np(P)), mref.project_bound(_np(dW0), _np(P)), f"project n={n}")
    again = dW0.clone()
    L.call("gdl_mla_project", L.ptr(again), L.ptr(P), n, L.cur_stream())
    assert _same(dW, again)


def test_project_refuses_513():
    dW, P = torch.full((513, 512), NAN, device=DEV), torch.full((512, 512), NAN, device=DEV)
    with pytest.raises(L.GdlError):
        L.call("gdl_mla_project", L.ptr(dW), L.ptr(P), 513, L.cur_stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dW).all()) and bool(torch.isnan(P).all())


# ------------------------------------------------------------------ gdl_mla_fuse
def _fuse_case(B, n):
    """Logit sets with the special rows the size has room for: 0 equal sets, 1 near one-hot (gap 200), 2 magnitude 1e4, 3 a NaN"""
    gen = torch.Generator(device=DEV).manual_seed(500 * B + n)
    a = 2 * torch.randn(B, n, generator=gen, device=DEV)
    v = 3 * torch.randn(B, n, generator=gen, device=DEV)
    v[0] = a[0]
    if B > 1:
        a[1] = 0.0
        a[1, n // 2] = 200.0
    if B > 2:
        a[2] *= 5e3
        v[2] *= 5e3
    if B > 3:
        v[3, n - 1] = NAN
    return a, v


def _fuse(a, v, dynamic, want_lam=True):
    B, n = a.shape
    out = torch.full((B, n), 7.0, device=DEV)
    lam = torch.full((B, 2), 7.0, device=DEV) if want_lam else None
    L.call("gdl_mla_fuse", L.ptr(a), L.ptr(v), B, n, int(dynamic), L.ptr(out), L.ptr(lam), L.cur_stream())
    return out, lam


@pytest.mark.parametrize("dynamic", [0, 1])
@pytest.mark.parametrize("B,n", [(1, 6), (5, 34), (65, 309), (257, 400)])
def test_fuse(B, n, dynamic):
    a, v = _fuse_case(B, n)
    out, lam = _fuse(a, v, dynamic)
    out2, none = _fuse(a, v, dynamic, want_lam=False)
    assert none is None and _same(out, out2), "lam = NULL: out keeps its bits"
    ref_out, ref_lam, sa, _ = mref.fuse(_np(a), _np(v), bool(dynamic))
    ok = np.isfinite(_np(v)).all(axis=1) & np.isfinite(_np(a)).all(axis=1)
    bd = mref.fuse_bounds(_np(a), _np(v), bool(dynamic))
    g_out, g_lam = _np(out), _np(lam)
    _within(g_lam[ok], ref_lam[ok], bd["lam"][ok], f"fuse lam B={B} n={n} dynamic={dynamic}")
    _within(g_out[ok], ref_out[ok], bd["out"][ok], f"fuse out B={B} n={n} dynamic={dynamic}")
    assert g_lam[0, 0] == 0.5 and g_lam[0, 1] == 0.5, "equal sets: lam exactly 0.5"
    assert np.isfinite(g_out[ok]).all() and np.isfinite(g_lam[ok]).all()
    if B > 1 and dynamic:
        assert g_lam[1, 0] > 0.5  # the near-one-hot audio row has entropy 0: no NaN from its p = 0 terms
    if B > 3:
        assert not ok[3] and not np.isfinite(g_out[3]).all()
        if dynamic:
            assert np.isnan(g_out[3]).all() and np.isnan(g_lam[3]).all()
    if not dynamic:
        assert np.all(g_lam == 0.5)


def test_fuse_refusals():
    a = torch.zeros(2, 513, device=DEV)
    out = torch.full((2, 513), NAN, device=DEV)
    with pytest.raises(L.GdlError):
        L.call("gdl_mla_fuse", L.ptr(a), L.ptr(a), 2, 513, 1, L.ptr(out), None, L.cur_stream())
    with pytest.raises(L.GdlError):
        L.call("gdl_mla_fuse", L.ptr(a), None, 2, 6, 1, L.ptr(out), None, L.cur_stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------ the runner
_STATE = {}


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def _state():
    """the seeded state make_golden_mla.py loads by name: generated once, shared, never modified"""
    if not _STATE:
        P, Bf = fx.model_state(6, "concat_dgl")
        st = {k: v for k, v in {**P, **Bf}.items() if k.startswith(("audio_net.", "visual_net."))}
        st.update(fx.make_state({"classifier.weight": (6, 512), "classifier.bias": (6,)}))
        _STATE.update({k: torch.from_numpy(np.array(v)) for k, v in st.items()})
    return _STATE


def _make_model(dtype="f32", batch=4):
    from models.basic_model import AVClassifier_MLA

    model = AVClassifier_MLA(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=batch))
    model.load_state_dict(_state(), strict=True)
    model = model.to(DEV)
    model.audio_net.gdl_dtype = model.visual_net.gdl_dtype = dtype
    return model.train()


_CFG = dict(seed=0, batch=4, spec_hw=[65, 47], frames=2, image_hw=[64, 64], n_classes=6)


def _batch(st, cfg=_CFG):
    spec, image, label = fx.make_batch(cfg["seed"] + st, cfg["batch"], cfg["spec_hw"], cfg["frames"], cfg["image_hw"],
                                       cfg["n_classes"])
    return dev(spec), dev(image), torch.from_numpy(label).to(DEV)


def _trainer(model=None, **kw):
    from gdl.mla import MLATrainer

    return MLATrainer(model if model is not None else _make_model(), lr=2e-3, **kw)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["mla_plain_tiny_b4", "mla_gs_tiny_b4"])
def test_mla_step_golden(name, dtype):
    """MLATrainer against the literal torch loop, half-step for half-step, with the constants of test_unimodal_step_golden
    (tests/test_unimodal_gpu.py) unchanged: `later` is the second batch.  In f32 the recorded parts of P are held to the bound
    mla_ref carries through the three shaped updates: the roundings of either side plus the measured difference between the
    runner's feature means and the recorded ones."""
    import gdl

    g = _gold(name)
    cfg = json.loads(str(g["config"]))
    model = _make_model(dtype)
    tr = _trainer(model, shaping=cfg["shaping"], normalize=cfg["normalize"])
    assert tr.names[60:62] == ["classifier.weight", "classifier.bias"] and len(tr.names) == 122
    f32 = dtype == "f32"
    rs, drs, alphas = [], [], []
    for st in range(cfg["steps"]):
        spec, image, label = _batch(st, cfg)
        tr.shaping_alpha = gdl.mla_alpha(st, cfg["steps_per_epoch"])
        tr.step(spec, image, label)
        r = tr.read()
        later = st > 0
        for m in ("audio", "visual"):
            pre = f"s{st}.{m[0]}."
            h = _np(tr.f[m])
            rs.append(g[pre + "r"].astype(np.float64))
            drs.append(np.abs(mref.feature_mean(h) - rs[-1]) + 2 * mref.feature_mean_bound(h))
            alphas.append(float(g[pre + "alpha"]))
            s, out, loss = r[m], r["out_" + m[0]], r["loss_" + m[0]]
            absent, present = ("visual_grad_sum", "audio_grad_sum") if m == "audio" else ("audio_grad_sum", "visual_grad_sum")
            assert s[absent] == 0.0 and float(g[pre + absent]) == 0.0
            if later and not f32:
                assert np.isfinite(out).all() and np.isfinite(s["total_norm"])
                continue
            lt = (1e-2 if later else 5e-4) if f32 else 0.2
            ls = lt if f32 else 5e-2
            print(name, dtype, pre, "logits", float(np.abs(out - g[pre + "out"]).max()), "loss", loss, float(g[pre + "loss_f"]),
                  "total_norm", s["total_norm"], float(g[pre + "total_norm"]), present, s[present], float(g[pre + present]))
            np.testing.assert_allclose(out, g[pre + "out"], rtol=lt, atol=lt)
            np.testing.assert_allclose(loss, g[pre + "loss_f"], rtol=ls, atol=ls)
            nt = (2e-2 if later else 3e-3) if f32 else 4e-2
            tn = float(g[pre + "total_norm"])
            np.testing.assert_allclose(s["total_norm"], tn, rtol=nt)
            np.testing.assert_allclose(s[present], g[pre + present], rtol=2 * nt)
            names = [str(n) for n in g[pre + "grad_names"]]
            gt = (6e-2 if later else 1e-2) if f32 else 0.3
            clip = min(1.0, 40.0 / (tn + 1e-6))
            worst = 0.0
            for i, n in enumerate(names):
                if g[pre + "grad_is_none"][i]:
                    assert n not in s["grad_norm"]
                    continue
                want = float(g[pre + "grad_norm"][i]) * clip
                worst = max(worst, abs(s["grad_norm"][n] - want) / (want + 1e-30))
                assert abs(s["grad_norm"][n] - want) <= gt * want + 1e-5 * clip * tn, (n, s["grad_norm"][n], want)
            print(name, dtype, pre, "worst per-tensor norm deviation", worst)
    last = f"s{cfg['steps'] - 1}.v."
    names = [str(n) for n in g[last + "grad_names"]]
    ps = g[last + "param_sums"]
    sd = model.state_dict()
    for i, n in enumerate(names):
        got = sd[n].double().abs().sum().item()
        np.testing.assert_allclose(got, ps[i][1], rtol=1e-3 if f32 else 2e-3, err_msg=n)
    for k in [k[len(last + "buf."):] for k in g.files if k.startswith(last + "buf.")]:
        tolr, tola = (2e-3, 1e-3) if f32 else (5e-2, 3e-2)
        np.testing.assert_allclose(sd[k].cpu().numpy().astype(np.float64), g[last + "buf." + k], rtol=tolr, atol=tola, err_msg=k)
    if f32:
        P = _np(tr.P)
        if not cfg["shaping"]:
            assert np.array_equal(P, np.eye(512, dtype=np.float32)) and np.array_equal(g[last + "Pdiag"], np.ones(512, np.float32))
        else:
            # update i of the run went against the mean of half-step i: three updates, the last half-step's mean is unused
            P64, b_run = mref.replay_projector(rs[:3], alphas[1:], drs=drs[:3])
            _, b_gold = mref.replay_projector(rs[:3], alphas[1:], any_order_norm=True)
            bound = b_run + b_gold
            print(name, "P: largest bound", float(bound.max()), "largest |P - P64|", float(np.abs(P - P64).max()))
            assert np.array_equal(P, P.T)
            # the whole P against the float64 replay: this side's roundings and the measured feature-mean differences alone
            print(name, "P against the replay: worst share of the bound", float((np.abs(P - P64) / b_run).max()))
            assert np.all(np.abs(P - P64) <= b_run)
            # the recorded parts: both sides' bounds (the torch loop's norm is summed in an order this test cannot know, which
            # costs gamma over all 262 144 terms per update and dominates the sum)
            assert np.all(np.abs(P[:16, :16] - g[last + "P16"]) <= bound[:16, :16])
            assert np.all(np.abs(np.diag(P) - g[last + "Pdiag"]) <= np.diag(bound))
            assert np.all(np.abs(P.astype(np.float64).sum(axis=1) - g[last + "Prowsum"]) <= bound.sum(axis=1))
            assert abs(float(np.sqrt((P.astype(np.float64) ** 2).sum())) - float(g[last + "Pfro"])) <= np.sqrt((bound ** 2).sum())
    model.eval()
    spec, image, label = _batch(1000, cfg)
    with torch.no_grad():
        _, ea, ev = model(spec.unsqueeze(1), image)
    et = 1e-2 if f32 else 0.2
    np.testing.assert_allclose(ea.cpu().numpy(), g["eval.out_a"], rtol=et, atol=et)
    np.testing.assert_allclose(ev.cpu().numpy(), g["eval.out_v"], rtol=et, atol=et)
    tr.close()


def test_audio_half_step_equals_unimodal_step():
    """shaping off, max_norm = 1e30 (the clip coefficient exactly 1, so the differently ordered norm sums of the two arena
    layouts cannot reach the update): the first audio half-step leaves the audio encoder, the head, their momentum and the
    BatchNorm buffers with the bits of one UnimodalTrainer audio step from the same state."""
    from gdl.unimodal import UnimodalTrainer
    from models.basic_model import AVClassifier_DGL

    spec, image, label = _batch(0)
    mm = _make_model()
    tm = _trainer(mm, shaping=False, max_norm=1e30)
    um = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="audio", batch_size=4))
    st = {k: v for k, v in _state().items() if k.startswith("audio_net.")}
    st.update({"audio_classifier.weight": _state()["classifier.weight"], "audio_classifier.bias": _state()["classifier.bias"]})
    st.update({k: v for k, v in um.state_dict().items() if k.startswith("fusion_module.")})
    um.load_state_dict(st, strict=True)
    um = um.to(DEV).train()
    um.audio_net.gdl_dtype = "f32"
    tu = UnimodalTrainer(um, lr=2e-3, max_norm=1e30)
    tm._half_step("audio", spec, image, label)
    tu.step(spec, None, label)
    rm, ru = tm.read(), tu.read()
    assert rm["audio"]["clip_coef"] == 1.0 and ru["clip_coef"] == 1.0
    assert _same(tm.df["audio"], tu.df) and _same(tm.outs["audio"], tu.out), "df carries UnimodalTrainer's bits"
    sm, su = mm.state_dict(), um.state_dict()
    for k in su:
        if k.startswith("audio_net."):
            assert _same(sm[k], su[k]) if sm[k].dtype == torch.float32 else torch.equal(sm[k], su[k]), k
    assert _same(sm["classifier.weight"], su["audio_classifier.weight"]) and _same(sm["classifier.bias"], su["audio_classifier.bias"])
    na, nh = tm.offsets[60], tm.offsets[62] - tm.offsets[60]
    assert _same(tm.momentum[:na], tu.momentum[nh:]) and _same(tm.momentum[na:na + nh], tu.momentum[:nh])
    assert float(tm.momentum[na + nh:].abs().max()) == 0.0
    tm.close()
    tu.close()


def test_inactive_encoder_untouched():
    """An audio half-step alone leaves the visual range of the parameter and momentum arenas unchanged bit for bit (no weight
    decay, no momentum drift), and a visual one the audio range -- after a full step, so that the momentum is not zero."""
    tr = _trainer()
    tr.step(*_batch(0))
    a0, a1, v0 = 0, tr.offsets[60], tr.offsets[62]
    spec, image, label = _batch(1)
    for m, lo, hi in (("audio", v0, tr.total), ("visual", a0, a1)):
        torch.cuda.synchronize()
        p, mo = tr.params[lo:hi].clone(), tr.momentum[lo:hi].clone()
        hp = tr.params[a1:v0].clone()
        assert float(mo.abs().max()) > 0.0
        tr._half_step(m, spec, image, label)
        torch.cuda.synchronize()
        assert _same(p, tr.params[lo:hi]) and _same(mo, tr.momentum[lo:hi]), m
        assert not _same(hp, tr.params[a1:v0]), "the head steps in every half-step"
    tr.close()


def test_valid():
    import gdl

    tr = _trainer()
    tr.step(*_batch(0))
    batches = [_batch(1000), _batch(1001)]
    for dynamic in (True, False):
        num, hit = np.zeros(6), np.zeros((3, 6))
        for b in batches:
            tr.valid([b], dynamic=dynamic)
            oa, ov, out, lab = _np(tr.outs["audio"]), _np(tr.outs["visual"]), _np(tr.out), _np(b[2])
            ref_out, ref_lam, _, _ = mref.fuse(oa, ov, dynamic)
            bd = mref.fuse_bounds(oa, ov, dynamic)
            assert np.all(np.abs(out - ref_out) <= bd["out"]) and np.all(np.abs(_np(tr.lam) - ref_lam) <= bd["lam"])
            for i, o in enumerate((out, oa, ov)):
                pred = torch.from_numpy(o).argmax(dim=1).numpy()
                np.add.at(hit[i], lab, pred == lab)
            np.add.at(num, lab, 1)
        bank = gdl.ScoreBank(6, 8, sets=3, device=DEV)
        acc = tr.valid(batches, bank=bank, dynamic=dynamic)
        assert np.array_equal(tr.valid_counts, np.concatenate([num[None], hit]))
        assert acc == tuple(hit[i].sum() / num.sum() for i in range(3))
        rep = bank.report(ks=(1,))
        assert rep["N"] == 8 and rep["topk"][1][0] == acc[0] and rep["topk"][1][1] == acc[1] and rep["topk"][1][2] == acc[2]
    tr.close()


def _arena_bytes(tr):
    torch.cuda.synchronize()
    return [t.clone() for t in (tr.params, tr.momentum, tr.P, tr.r_prev)] + \
        [v.clone() for k, v in tr.model.state_dict().items() if "running_" in k or "num_batches" in k]


def _all_same(x, y):
    return all(_same(a, b) if a.dtype == torch.float32 else torch.equal(a, b) for a, b in zip(x, y))


def test_determinism_and_checkpoint():
    """Two fresh trainers leave identical bytes in the arenas and P after two batches; two batches, save, two more equals load,
    two more, bit for bit, P included."""
    import copy

    runs = []
    for _ in range(2):
        tr = _trainer()
        for st in range(2):
            tr.step(*_batch(st))
        runs.append(tr)
    assert _all_same(_arena_bytes(runs[0]), _arena_bytes(runs[1]))
    assert not _same(runs[0].P, torch.eye(512, device=DEV)) and _same(runs[0].P, runs[0].P.t())
    a, b = runs
    ck_model = copy.deepcopy({k: v.clone() for k, v in a.model.state_dict().items()})
    ck = a.state_dict()
    assert ck["have_prev"] == 1 and _same(ck["P"], a.P)
    for st in (2, 3):
        a.step(*_batch(st))
    # b is overwritten with zeros first, so that everything it ends with came through the checkpoint
    b.momentum.zero_()
    b.P.zero_()
    b.r_prev.zero_()
    b.have_prev = 0
    b.model.load_state_dict(ck_model)
    b.load_state_dict(ck)
    assert b.params.data_ptr() == b.pviews[0].data_ptr() and b.model.classifier.weight.data_ptr() == b.pviews[60].data_ptr()
    for st in (2, 3):
        b.step(*_batch(st))
    assert _all_same(_arena_bytes(a), _arena_bytes(b))
    bad = dict(ck)
    del bad["P"]
    with pytest.raises(L.GdlError):
        b.load_state_dict(bad)
    a.close()
    b.close()
    b.close()  # idempotent


def test_refusals():
    from gdl.mla import MLATrainer
    from models.basic_model import AVClassifier_DGL, AVClassifier_DGL_Swin, AVClassifier_MLA

    model = _make_model()
    for kw in (dict(optimizer="Adam"), dict(optimizer="AdaGrad"), dict(process_group=object()), dict(journal=8),
               dict(diversity=True), dict(modulation="OGM_GE"), dict(prototypes=object()), dict(shaping_alpha=0.0),
               dict(shaping_alpha=float("nan"))):
        with pytest.raises(L.GdlError):
            MLATrainer(model, lr=2e-3, **kw)
    ns = argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=4)
    with pytest.raises(L.GdlError):
        MLATrainer(AVClassifier_DGL(ns).to(DEV), lr=2e-3)
    with pytest.raises(L.GdlError):
        MLATrainer(AVClassifier_MLA(ns), lr=2e-3)  # a CPU model
    swin = AVClassifier_MLA(ns)
    swin.visual_net = AVClassifier_DGL_Swin(ns).visual_net
    with pytest.raises(L.GdlError):
        MLATrainer(swin.to(DEV), lr=2e-3)
    tr = MLATrainer(model, lr=2e-3)
    spec, image, label = _batch(0)
    with pytest.raises(L.GdlError):
        tr.step(spec.cpu(), image, label)
    with pytest.raises(L.GdlError):
        tr.step(spec, image.cpu(), label)
    with pytest.raises(L.GdlError):
        tr.step(spec, image, label.cpu())
    tr.shaping_alpha = -1.0
    with pytest.raises(L.GdlError):
        tr.step(spec, image, label)
    with pytest.raises(L.GdlError):
        tr._half_step("fused", spec, image, label)
    torch.cuda.synchronize()
    assert tr.steps == 0 and _same(tr.P, torch.eye(512, device=DEV))
    tr.close()
