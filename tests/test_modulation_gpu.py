"""GPU tests of OGM / OGM-GE gradient modulation (main.py --modulation, :286-330) on the joint-training runner: the score
kernel and the arena modulation against the float64 restatement of tests/modulation_ref.py (pinned on the CPU by
tests/test_modulation_cpu.py), the three update kernels behind it, DGLTrainer(mode="joint", modulation=...) against a Normal
trainer, against the reference's OGM step goldens (tests/golden/make_golden_ogm.py), the switch-off cases, checkpoints and the
refusals."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import modulation_ref as mref  # noqa: E402
import optim_ref as oref  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev  # noqa: E402

from oracle import fixtures as fx  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL, ATOL_REL = 1e-5, 1e-6  # tests/test_optimizers_gpu.py's bounds of the update kernels against tests/optim_ref.py
ALPHA = 0.8


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Optim:
    """a gdl_optim_t over `sizes` with its workspaces, the modulation's included"""

    def __init__(self, sizes, group, marks):
        self.lib = L.load()
        self.offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.n = int(self.offs[-1])
        self.h = ctypes.c_void_p()
        L.call("gdl_optim_create", ctypes.byref(self.h), (ctypes.c_int64 * len(self.offs))(*self.offs.tolist()),
               (ctypes.c_int32 * len(group))(*group), len(group))
        self.wsb = self.lib.gdl_optim_workspace_bytes(self.h)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=DEV)
        self.stats = torch.zeros(self.lib.gdl_optim_stats_len(self.h), device=DEV)
        self.mwsb = self.lib.gdl_optim_modulate_workspace_bytes(self.h)
        self.mws = torch.empty(self.mwsb, dtype=torch.uint8, device=DEV)
        self.mstats = torch.full((self.lib.gdl_optim_modulate_stats_len(self.h),), float("nan"), device=DEV)
        self.marks = list(marks)
        L.call("gdl_optim_modulate_bind", self.h, (ctypes.c_int32 * len(marks))(*marks), L.ptr(self.mws), self.mwsb, L.cur_stream())

    def stats_pass(self, G, grad_scale):
        L.call("gdl_optim_grad_stats", self.h, L.ptr(G), 40.0, grad_scale, L.ptr(self.stats), L.ptr(self.ws), self.wsb,
               L.cur_stream())

    def modulate(self, G, grad_scale, scores, noise, seed=0, step=0):
        """statistics + modulation of G in place; returns (k, mod_stats) on the host"""
        self.stats_pass(G, grad_scale)
        L.call("gdl_optim_modulate", self.h, L.ptr(G), L.ptr(self.stats), grad_scale, L.ptr(scores), ALPHA, int(noise), seed, step,
               L.ptr(self.mstats), L.ptr(self.ws), L.ptr(self.mws), L.cur_stream())
        torch.cuda.synchronize()
        k = np.float32(self.stats[1].item()) * np.float32(grad_scale)
        return k, self.mstats.cpu().numpy()

    def close(self):
        self.lib.gdl_optim_destroy(self.h)


# ------------------------------------------------------------------ the score kernel
def _scores(layout, fa, fv, P, label, B, n):
    prob = torch.full((B, 2), float("nan"), device=DEV)
    scores = torch.full((2,), float("nan"), device=DEV)
    nb = L.load().gdl_head_uni_scores_workspace_bytes()
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    if layout == "concat":
        args = (L.ptr(P[0]), P[0].data_ptr() + 512 * 4, 1024, L.ptr(P[1]), L.ptr(P[1]), 0.5)
    else:
        args = (L.ptr(P[0]), L.ptr(P[2]), 512, L.ptr(P[1]), L.ptr(P[3]), 1.0)
    first = None
    for _ in range(2):  # twice on one workspace: the ticket counter comes back at zero, and the second run repeats the bits
        L.call("gdl_head_uni_scores", L.ptr(fa), L.ptr(fv), *args, L.ptr(label), L.ptr(prob), L.ptr(scores), B, n, L.ptr(ws), nb,
               L.cur_stream())
        if first is None:
            first = (prob.clone(), scores.clone())
            prob.fill_(float("nan")), scores.fill_(float("nan"))
    torch.cuda.synchronize()
    assert not ws.any()
    for a, c in zip(first, (prob, scores)):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    return prob, scores


@pytest.mark.parametrize("B,n", [(5, 6), (33, 34), (3, 309), (65, 6), (257, 6), (257, 34)])
@pytest.mark.parametrize("layout", ["concat", "sum"])
def test_score_kernel(layout, B, n):
    """gdl_head_uni_scores against NumPy float64 (rtol 1e-4: a 512-term fp32 dot through exp) for both weight layouts, with the
    inputs rebuilt so that each side leads once, and the coefficients the finalise kernel derives from the scores within
    1e-6 + 1e-4 |want| (1 - tanh cancels near 0).  309 classes: more than a wavefront is wide; the odd B: row tails; B = 65 and 257: more blocks than a
    wavefront has lanes and than one 256-sample lap, each run twice with bit-equal results."""
    r = np.random.default_rng([5, B, n, layout == "sum"])
    shapes = ((n, 1024), (n,)) if layout == "concat" else ((n, 512), (n,), (n, 512), (n,))
    Pn = [(r.standard_normal(s) * (0.05 if len(s) == 2 else 0.1)).astype(np.float32) for s in shapes]
    label = r.integers(0, n, B)
    Wa, Wv = (Pn[0][:, :512], Pn[0][:, 512:]) if layout == "concat" else (Pn[0], Pn[2])
    opt = _Optim([8], [1], [1])
    seen = set()
    try:
        for lead in ("audio", "visual"):
            fa = np.maximum(r.standard_normal((B, 512)), 0).astype(np.float32)
            fv = np.maximum(r.standard_normal((B, 512)), 0).astype(np.float32)
            if lead == "audio":  # push the leading side's logit of the label up
                fa += 2 * Wa[label]
            else:
                fv += 2 * Wv[label]
            P = [dev(p) for p in Pn]
            prob, scores = _scores(layout, dev(fa), dev(fv), P, torch.from_numpy(label).to(DEV), B, n)
            ua, uv = mref.uni_logits(layout, fa, fv, Pn)
            want = np.stack([mref.label_probs(ua, label), mref.label_probs(uv, label)], axis=1)
            np.testing.assert_allclose(prob.cpu().numpy(), want, rtol=1e-4)
            np.testing.assert_allclose(scores.cpu().numpy(), want.sum(0), rtol=1e-4)
            _, ms = opt.modulate(torch.ones(8, device=DEV), 1.0, scores, False)
            rv, ca, cv = mref.coefficients(want[:, 0].sum(), want[:, 1].sum(), ALPHA)
            assert (rv > 1) == (lead == "visual")
            np.testing.assert_array_equal(ms[:2], scores.cpu().numpy())
            np.testing.assert_allclose(ms[2], rv, rtol=2e-4)
            for got, w in ((ms[3], ca), (ms[4], cv)):
                assert abs(got - w) <= 1e-6 + 1e-4 * abs(w), (lead, got, w)
            assert (ms[4] == 1.0) == (lead == "audio") and (ms[3] == 1.0) == (lead == "visual")
            seen.add(lead)
        assert seen == {"audio", "visual"}
        # a label outside [0, n) poisons the sample's probabilities and both scores, as the loss kernels do
        bad = torch.from_numpy(label).to(DEV)
        bad[B - 1] = n
        prob, scores = _scores(layout, dev(fa), dev(fv), P, bad, B, n)
        assert torch.isnan(prob[B - 1]).all() and torch.isfinite(prob[:B - 1]).all() and torch.isnan(scores).all()
    finally:
        opt.close()


def test_ratio_one_takes_the_audio_branch_on_the_device():
    opt = _Optim([8], [1], [2])
    try:
        _, ms = opt.modulate(torch.ones(8, device=DEV), 1.0, torch.tensor([1.25, 1.25], device=DEV), False)
        assert ms[2] == 1.0 and ms[4] == 1.0 and abs(ms[3] - (1 - np.tanh(ALPHA))) <= 1e-6 + 1e-4 * (1 - np.tanh(ALPHA))
    finally:
        opt.close()


# ------------------------------------------------------------------ the modulation over the arena
SIZES = [6144, 6, 3136, 64, 64, 36864, 9, 147456, 8196]  # test_update_op's arena: length = 3 mod 4, unaligned segment starts
GROUP = [0, 0, 1, 1, 1, 1, 2, 2, 2]
MARKS = [0, 0, 1, 0, 0, 1, 0, 2, 2]


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("scale", [0.01, 10.0])  # below / above the clipping threshold
def test_modulate_op(scale, grad_scale):
    """gdl_optim_modulate behind gdl_optim_grad_stats: (a) unmarked segments as the Normal path writes them, bit for bit;
    (b) OGM: float32(float32(g k) c) bit for bit, each side leading once; (c) OGM_GE: sigma against float64 at rtol 1e-5;
    (d) the noise (G - (g k) c) / sigma against the reference normals within 1e-3 (a wrong counter, lane or segment is off by
    O(1), float32 rounding is ~1e-6); (e) reproducible in (seed, step), different for another step or seed; and the three update
    kernels behind it (stats = NULL, grad_scale = 1) against tests/optim_ref.py from the modulated gradient."""
    opt = _Optim(SIZES, GROUP, MARKS)
    offs, n = opt.offs, opt.n
    assert n % 4 == 3
    r = np.random.default_rng([43, int(scale * 100), int(grad_scale * 10)])
    g = (scale * r.standard_normal(n)).astype(np.float32)
    marked = np.zeros(n, dtype=bool)
    for s, m in enumerate(MARKS):
        marked[offs[s]:offs[s + 1]] = m != 0
    lr = 2e-3
    try:
        # the Normal path: statistics + SGD, which writes g k back where k != 1
        Gn, P, M = dev(g), dev(r.standard_normal(n).astype(np.float32)), torch.zeros(n, device=DEV)
        opt.stats_pass(Gn, grad_scale)
        L.call("gdl_optim_sgd_step", opt.h, L.ptr(P), L.ptr(Gn), L.ptr(M), L.ptr(opt.stats), grad_scale, lr, 0.9, 1e-4,
               L.cur_stream())
        torch.cuda.synchronize()
        assert (opt.stats[1].item() < 1.0) == (scale > 1.0)
        normal = Gn.cpu().numpy()
        for sc in ((1.0, 1.3), (1.3, 1.0)):  # visual leads / audio leads
            scores = torch.tensor(sc, device=DEV)
            G = dev(g)
            k, ms = opt.modulate(G, grad_scale, scores, False)
            got = G.cpu().numpy()
            gk = g * k
            np.testing.assert_array_equal(gk, normal)  # (what the Normal path holds: g k, or g untouched where k == 1)
            np.testing.assert_array_equal(got[~marked].view(np.int32), normal[~marked].view(np.int32))  # (a)
            assert (ms[3] == 1.0) == (sc[1] > sc[0]) and (ms[4] == 1.0) == (sc[1] <= sc[0]) and not ms[8:].any()
            for s, m in enumerate(MARKS):  # (b)
                if m:
                    c = np.float32(ms[2 + m])
                    np.testing.assert_array_equal(got[offs[s]:offs[s + 1]].view(np.int32), (gk[offs[s]:offs[s + 1]] * c).view(np.int32))
        # OGM_GE
        seed, step = 0x0123456789abcdef, 7
        G = dev(g)
        k, ms = opt.modulate(G, grad_scale, scores, True, seed, step)
        ge = G.cpu().numpy()
        gk = g * k
        ca, cv = float(ms[3]), float(ms[4])
        _, sig = mref.modulate(g, offs, MARKS, k, ca, cv, True, seed, step)
        np.testing.assert_array_equal(ge[~marked].view(np.int32), normal[~marked].view(np.int32))  # (a)
        worst = 0.0
        for s, m in enumerate(MARKS):
            b, e = offs[s], offs[s + 1]
            if not m:
                assert ms[8 + s] == 0.0
                continue
            np.testing.assert_allclose(ms[8 + s], sig[s], rtol=1e-5)  # (c)
            c = np.float32(ms[2 + m])
            z = (ge[b:e].astype(np.float64) - (gk[b:e] * c).astype(np.float64)) / float(ms[8 + s])
            err = float(np.abs(z - mref.normals(np.arange(b, e, dtype=np.int64), seed, step)).max())
            worst = max(worst, err)
            assert err < 1e-3, (s, err)  # (d)
        print("modulate_op", scale, grad_scale, "k", k, "worst noise deviation (sigma units)", worst)
        G2 = dev(g)  # (e)
        opt.modulate(G2, grad_scale, scores, True, seed, step)
        assert _same_bits(G, G2)
        for sd, stp in ((seed, step + 1), (seed + 1, step), (seed + (1 << 32), step)):
            G3 = dev(g)
            opt.modulate(G3, grad_scale, scores, True, sd, stp)
            assert _same_bits(G3[~torch.from_numpy(marked).to(DEV)], G[~torch.from_numpy(marked).to(DEV)])
            assert not torch.equal(G3, G)
        # the update kernels behind the modulation take the arena as it stands and leave it alone
        gm = ge.astype(np.float64)
        p0 = r.standard_normal(n).astype(np.float32)
        for kind in ("sgd", "Adam", "AdaGrad"):
            Pk, S1, S2 = dev(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
            st = L.cur_stream()
            if kind == "sgd":
                L.call("gdl_optim_sgd_step", opt.h, L.ptr(Pk), L.ptr(G), L.ptr(S1), None, 1.0, lr, 0.9, 1e-4, st)
                m = gm + 1e-4 * p0
                wp, ws1 = p0 - lr * m, m
            elif kind == "Adam":
                L.call("gdl_optim_adamw_step", opt.h, L.ptr(Pk), L.ptr(G), L.ptr(S1), L.ptr(S2), None, 1.0, lr, 0.9, 0.999, 1e-8,
                       1e-2, 1, st)
                wp, ws1, ws2 = oref.adamw(p0.astype(np.float64), gm, np.zeros(n), np.zeros(n), lr, 1, weight_decay=1e-2)
            else:
                L.call("gdl_optim_adagrad_step", opt.h, L.ptr(Pk), L.ptr(G), L.ptr(S1), None, 1.0, lr, 1e-10, 1e-2, 1, st)
                wp, ws1 = oref.adagrad(p0.astype(np.float64), gm, np.zeros(n), lr, weight_decay=1e-2)
            torch.cuda.synchronize()
            np.testing.assert_allclose(Pk.cpu().numpy(), wp, rtol=RTOL, atol=ATOL_REL * float(np.abs(wp).max()), err_msg=kind)
            np.testing.assert_allclose(S1.cpu().numpy(), ws1, rtol=RTOL, atol=ATOL_REL * float(np.abs(ws1).max()), err_msg=kind)
            if kind == "Adam":
                np.testing.assert_allclose(S2.cpu().numpy(), ws2, rtol=RTOL, atol=ATOL_REL * float(np.abs(ws2).max()), err_msg=kind)
            np.testing.assert_array_equal(G.cpu().numpy(), ge)
    finally:
        opt.close()


def test_modulate_refusals():
    """A marked segment of fewer than 2 elements (the unbiased standard deviation divides by n - 1), a mark outside {0, 1, 2}, a
    workspace that is too small or was never bound."""
    lib = L.load()
    h = ctypes.c_void_p()
    L.call("gdl_optim_create", ctypes.byref(h), (ctypes.c_int64 * 3)(0, 1, 9), (ctypes.c_int32 * 2)(1, 2), 2)
    try:
        nb = lib.gdl_optim_modulate_workspace_bytes(h)
        assert nb > 0 and lib.gdl_optim_modulate_stats_len(h) == 8 + 2
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        for marks in ((1, 2), (0, 3)):
            with pytest.raises(L.GdlError):
                L.call("gdl_optim_modulate_bind", h, (ctypes.c_int32 * 2)(*marks), L.ptr(ws), nb, L.cur_stream())
        with pytest.raises(L.GdlError):
            L.call("gdl_optim_modulate_bind", h, (ctypes.c_int32 * 2)(0, 2), L.ptr(ws), nb - 1, L.cur_stream())
        G, stats, sc, ms = (torch.ones(k, device=DEV) for k in (12, 8, 2, 10))
        ows = torch.empty(lib.gdl_optim_workspace_bytes(h), dtype=torch.uint8, device=DEV)
        L.call("gdl_optim_grad_stats", h, L.ptr(G), 40.0, 1.0, L.ptr(stats), L.ptr(ows), ows.numel(), L.cur_stream())
        with pytest.raises(L.GdlError):  # never bound
            L.call("gdl_optim_modulate", h, L.ptr(G), L.ptr(stats), 1.0, L.ptr(sc), ALPHA, 0, 0, 0, L.ptr(ms), L.ptr(ows), L.ptr(ws),
                   L.cur_stream())
        torch.cuda.synchronize()
    finally:
        lib.gdl_optim_destroy(h)


# ------------------------------------------------------------------ the runner
_STATE = {}
_TINY = dict(dataset="CREMAD", n_classes=6, spec_hw=[65, 47], frames=2, image_hw=[64, 64], batch=4, seed=0, lr=2e-3)
_FIXSTATE = {"concat": "concat", "sum": "sum_dgl"}  # the fixture states of tests/golden/make_golden_ogm.py


def _state(n_classes, fusion):
    if (n_classes, fusion) not in _STATE:
        P, Bf = fx.model_state(n_classes, _FIXSTATE[fusion])
        _STATE[(n_classes, fusion)] = {k: torch.from_numpy(np.array(v)) for k, v in {**P, **Bf}.items()}
    return _STATE[(n_classes, fusion)]


def _make_model(cfg, dtype):
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


def _head_params(tr):
    return [p.detach().cpu().numpy().copy() for p in tr.pviews[:tr.nf]]


def _want_ogm(tr, head, P0, label):
    """float64 scores and coefficients from the trainer's pooled features and the head parameters in front of the update"""
    ua, uv = mref.uni_logits(head, tr.fa.cpu().numpy(), tr.fv.cpu().numpy(), P0)
    lab = label.cpu().numpy()
    sa, sv = mref.label_probs(ua, lab).sum(), mref.label_probs(uv, lab).sum()
    return (sa, sv) + mref.coefficients(sa, sv, ALPHA)


@pytest.mark.parametrize("fusion", ["concat", "sum"])
def test_runner_three_modulations(fusion):
    """Normal, OGM and OGM_GE trainers from one state on one tiny batch, one f32 step: identical statistics and logits; OGM's
    convolution gradients are coeff * Normal's bit for bit; OGM_GE's differ from OGM's by sigma z (sigma of Normal's arena, z the
    reference's; within 1e-3 in sigma units, as the op test); BatchNorm and head gradients are equal; read()['ogm'] agrees with
    float64 from the trainer's features and parameters (scores rtol 1e-4, coefficients 1e-6 + 1e-4 |want|)."""
    cfg = dict(_TINY, fusion=fusion)
    spec, image, label = _batch(cfg, 0)
    seed = 12345
    runs = {}
    for mod in ("Normal", "OGM", "OGM_GE"):
        model, tr = _trainer(cfg, alpha=ALPHA, modulation=mod, seed=seed)
        P0 = _head_params(tr)
        tr.step(spec, image, label)
        runs[mod] = (model, tr, tr.read(), P0)
    trn, rn = runs["Normal"][1], runs["Normal"][2]
    assert "ogm" not in rn
    for mod in ("OGM", "OGM_GE"):
        _, tr, r, P0 = runs[mod]
        np.testing.assert_array_equal(r["out"], rn["out"])
        for k in ("total_norm", "clip_coef", "audio_grad_sum", "visual_grad_sum", "loss_f"):
            assert r[k] == rn[k], (mod, k)
        assert r["grad_norm"] == rn["grad_norm"] and r["grad_absmean"] == rn["grad_absmean"]
        sa, sv, rv, ca, cv = _want_ogm(tr, fusion, P0, label)
        o = r["ogm"]
        print(fusion, mod, o, "float64", sa, sv, rv, ca, cv)
        np.testing.assert_allclose([o["score_a"], o["score_v"], o["ratio_v"]], [sa, sv, rv], rtol=1e-4)
        for got, w in ((o["coeff_a"], ca), (o["coeff_v"], cv)):
            assert abs(got - w) <= 1e-6 + 1e-4 * abs(w), (mod, got, w)
    assert runs["OGM"][2]["ogm"] == runs["OGM_GE"][2]["ogm"]
    tro, trg = runs["OGM"][1], runs["OGM_GE"][1]
    coef = {1: tro.mod_stats[3], 2: tro.mod_stats[4]}
    nconv = 0
    for i, name in enumerate(trn.names):
        gn, go, gg = trn.grad(name), tro.grad(name), trg.grad(name)
        side = 1 if name.startswith("audio_net.") else (2 if name.startswith("visual_net.") else 0)
        if side and gn.dim() == 4:
            nconv += 1
            assert _same_bits(go, gn * coef[side]), name
            sig = mref.sigma(gn.cpu().numpy())
            z = (gg.double() - go.double()).cpu().numpy().reshape(-1) / sig
            zr = mref.normals(np.arange(trn.offsets[i], trn.offsets[i + 1], dtype=np.int64), seed, 0)
            assert float(np.abs(z - zr).max()) < 1e-3, name
        else:
            assert _same_bits(go, gn) and _same_bits(gg, gn), name
    assert nconv == 40
    for _, tr, _, _ in runs.values():
        tr.close()


GOLDENS = ["ogm_concat_tiny_b4", "ogm_sum_tiny_b4"]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", GOLDENS)
def test_ogm_step_golden(name, dtype):
    """DGLTrainer(mode="joint", modulation="OGM") against the reference's OGM step (two steps: each side leads once).  f32: per
    step the logits, loss, total norm, gradient sums and per-tensor norms -- of the clipped, unmodulated gradient -- and the final
    parameter sums, buffers and eval logits to the constants of tests/test_joint_gpu.py::test_joint_step_golden; step-0 scores
    within 1e-3 absolute (|dp| <= max|dlogit| / 2 per sample, times B = 4, at that test's 5e-4 logit bound), coefficients within
    alpha (1 + ratio) 1e-3 / min(score_a, score_v) (|d(1 - tanh)/dx| <= 1 and the quotient rule), the leading side at both
    steps.  bf16: everything finite and the leading side."""
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    cfg = json.loads(str(g["config"]))
    assert cfg["modulation"] == "OGM" and cfg["alpha"] == ALPHA and cfg["steps"] == 2
    model, tr = _trainer(cfg, dtype, alpha=cfg["alpha"], modulation="OGM", modulation_starts=cfg["modulation_starts"],
                         modulation_ends=cfg["modulation_ends"])
    f32 = dtype == "f32"
    leads = []
    for st in range(cfg["steps"]):
        spec, image, label = _batch(cfg, st)
        tr.step(spec, image, label)
        r = tr.read()
        pre = f"s{st}."
        later = st > 0
        o = r["ogm"]
        want = {k: float(g[pre + k]) for k in ("score_a", "score_v", "ratio_v", "coeff_a", "coeff_v")}
        print(name, dtype, st, o, "golden", want)
        leads.append(want["ratio_v"] > 1)
        assert all(np.isfinite(v) for v in o.values())
        assert (o["ratio_v"] > 1) == (want["ratio_v"] > 1), (st, o, want)
        assert (o["coeff_v"] < 1) == (want["ratio_v"] > 1) and (o["coeff_a"] < 1) == (not want["ratio_v"] > 1)
        if not f32:
            assert np.isfinite(r["out"]).all() and np.isfinite(r["total_norm"]) and np.isfinite(r["loss_f"])
            continue
        if not later:
            assert abs(o["score_a"] - want["score_a"]) < 1e-3 and abs(o["score_v"] - want["score_v"]) < 1e-3
            ratio = max(want["ratio_v"], 1.0 / want["ratio_v"])
            ctol = cfg["alpha"] * (1 + ratio) * 1e-3 / min(want["score_a"], want["score_v"])
            assert abs(o["coeff_a"] - want["coeff_a"]) <= ctol and abs(o["coeff_v"] - want["coeff_v"]) <= ctol
        lt = 1e-2 if later else 5e-4
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


def test_ogm_moves_the_parameters_like_the_golden():
    """The momentum the golden recorded carries the MODULATED gradient (first step: momentum = g + wd p): the runner's sum of
    |momentum| per tensor matches it to 1e-2 (test_joint_step_golden's first-step per-tensor bound) -- plus, for the slowed side's
    convolution weights, the coefficient's relative bound: |d ln(1 - tanh x)| <= 2 |dx|, x = alpha ratio, d ratio <=
    (1 + ratio) 1e-3 / min(score) as in test_ogm_step_golden.  Here ratio_v = 2.41: the visual gradients shrink 24-fold, which
    no such bound could hide."""
    g = np.load(os.path.join(GOLD, "ogm_sum_tiny_b4.npz"), allow_pickle=False)
    cfg = json.loads(str(g["config"]))
    model, tr = _trainer(cfg, "f32", alpha=cfg["alpha"], modulation="OGM")
    tr.step(*_batch(cfg, 0))
    torch.cuda.synchronize()
    names = [str(n) for n in g["s0.grad_names"]]
    rv, cv = float(g["s0.ratio_v"]), float(g["s0.coeff_v"])
    assert rv > 1 and cv < 0.1
    ctol = 2 * cfg["alpha"] * (1 + rv) * 1e-3 / min(float(g["s0.score_a"]), float(g["s0.score_v"]))
    worst = 0.0
    for i, n in enumerate(names):
        j = tr.names.index(n)
        got = tr.momentum[tr.offsets[j]:tr.offsets[j + 1]].double().abs().sum().item()
        want = float(g["s0.momentum_sums"][i][1])
        slowed = n.startswith("visual_net.") and tr.pviews[j].dim() == 4
        worst = max(worst, abs(got - want) / want)
        assert abs(got - want) <= (1e-2 + (ctol if slowed else 0.0)) * want + 1e-9, (n, got, want)
    print("worst momentum-sum deviation", worst, "slowed-side allowance", ctol)
    tr.close()


@pytest.mark.parametrize("how", ["Normal", "window"])
def test_switched_off_is_bit_identical(how):
    """modulation="Normal", or an epoch outside the window, is the step of a trainer built without the new arguments, bit for
    bit: parameters, gradients, momentum, statistics -- over two steps."""
    cfg = dict(_TINY, fusion="concat")
    from gdl.trainer import DGLTrainer

    m0 = _make_model(cfg, "f32")
    t0 = DGLTrainer(m0, lr=cfg["lr"], mode="joint")
    kw = dict(modulation="Normal", alpha=ALPHA) if how == "Normal" else \
        dict(modulation="OGM_GE", alpha=ALPHA, modulation_starts=2, modulation_ends=3)
    m1, t1 = _trainer(cfg, **kw)
    for st in range(2):  # (window: the default epoch 0 is in front of it, epoch 4 behind)
        b = _batch(cfg, st)
        t0.step(*b)
        t1.step(*b)
        if how == "window" and st == 0:
            t1.epoch = 4
        r0, r1 = t0.read(), t1.read()
        assert "ogm" not in r1
        np.testing.assert_array_equal(r0["out"], r1["out"])
        assert _same_bits(t0.stats, t1.stats) and _same_bits(t0.grads, t1.grads)
        assert _same_bits(t0.params, t1.params) and _same_bits(t0.momentum, t1.momentum)
    sd = t1.state_dict()
    assert ("modulation" in sd) == (how == "window")
    t0.close()
    t1.close()


def test_window_switches_the_modulation_on():
    """inside the window the same trainer modulates: read() reports it and the convolution gradients shrink"""
    cfg = dict(_TINY, fusion="sum")
    _, t = _trainer(cfg, modulation="OGM", alpha=ALPHA, modulation_starts=1, modulation_ends=1)
    t.step(*_batch(cfg, 0))
    assert "ogm" not in t.read()
    t.epoch = 1
    t.step(*_batch(cfg, 1))
    assert "ogm" in t.read()
    t.epoch = 2
    t.step(*_batch(cfg, 0))
    assert "ogm" not in t.read()
    t.close()


def test_checkpoint_continues_the_noise():
    """state_dict() after step 1 of an OGM_GE run: a fresh trainer continues steps 2 and 3 bit-identically (the step count drives
    the noise counter, the seed travels in the checkpoint); a checkpoint of another modulation is refused."""
    cfg = dict(_TINY, fusion="concat")
    m0, t0 = _trainer(cfg, modulation="OGM_GE", alpha=ALPHA, seed=99)
    t0.step(*_batch(cfg, 0))
    ck_model = {k: v.clone() for k, v in m0.state_dict().items()}
    ck = t0.state_dict()
    assert ck["modulation"] == "OGM_GE" and ck["seed"] == 99 and ck["steps"] == 1
    m1 = _make_model(cfg, "f32")
    m1.load_state_dict(ck_model)
    from gdl.trainer import DGLTrainer

    t1 = DGLTrainer(m1, lr=cfg["lr"], mode="joint", modulation="OGM_GE", alpha=ALPHA, seed=5)  # (the checkpoint's seed wins)
    t1.load_state_dict(ck)
    assert t1.steps == 1 and t1.seed == 99
    for st in (1, 2):
        b = _batch(cfg, st)
        t0.step(*b)
        t1.step(*b)
        r0, r1 = t0.read(), t1.read()
        assert r0["ogm"] == r1["ogm"] and r0["total_norm"] == r1["total_norm"]
        assert _same_bits(t0.grads, t1.grads) and _same_bits(t0.params, t1.params) and _same_bits(t0.momentum, t1.momentum)
    for k, v in m0.state_dict().items():
        assert torch.equal(v, m1.state_dict()[k]), k
    for other in ("Normal", "OGM"):
        m2, t2 = _trainer(cfg, modulation=other, alpha=ALPHA)
        with pytest.raises(L.GdlError, match="modulation"):
            t2.load_state_dict(ck)
        t2.close()
    plain = dict(ck)
    del plain["modulation"], plain["seed"]
    with pytest.raises(L.GdlError, match="modulation"):
        t1.load_state_dict(plain)
    t0.close()
    t1.close()


def test_refusals():
    """What the modulation is not built for raises instead of being ignored: an unknown name, mode="dgl", the gated and FiLM
    heads, the Swin branch, a process group."""
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier, AVClassifier_DGL, AVClassifier_DGL_Swin

    def ns(fusion):
        return argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality="full", batch_size=4)

    joint = AVClassifier(ns("concat")).to(DEV)
    with pytest.raises(ValueError, match="modulation"):
        DGLTrainer(joint, lr=1e-3, mode="joint", modulation="GE")
    for mod in ("OGM", "OGM_GE"):
        with pytest.raises(L.GdlError, match="joint"):
            DGLTrainer(AVClassifier_DGL(ns("concat")).to(DEV), lr=1e-3, mode="dgl", modulation=mod)
        with pytest.raises(L.GdlError, match="process group"):
            DGLTrainer(joint, lr=1e-3, mode="joint", modulation=mod, process_group=object())
    for fusion in ("gated", "film"):
        with pytest.raises(L.GdlError, match="concat and sum"):
            DGLTrainer(AVClassifier(ns(fusion)).to(DEV), lr=1e-3, mode="joint", modulation="OGM")
    sc = fx.SWIN_TINY2
    swin = AVClassifier_DGL_Swin(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", pe=0),
                                 swin_kwargs=dict(img_size=sc["img"], patch_size=sc["patch"], embed_dim=sc["embed"],
                                                  depths=list(sc["depths"]), num_heads=list(sc["heads"]),
                                                  window_size=sc["window"], mlp_ratio=float(sc["mlp"]), drop_path_rate=0.)).to(DEV)
    for mode in ("joint", "dgl"):
        with pytest.raises(L.GdlError):
            DGLTrainer(swin, lr=1e-3, mode=mode, modulation="OGM")
    # Normal is accepted everywhere it was
    DGLTrainer(AVClassifier_DGL(ns("concat")).to(DEV), lr=1e-3, mode="dgl", modulation="Normal").close()
