"""CPU-only checks of what the GPU tests of alternating unimodal training (MLA) are measured against (tests/mla_ref.py): the
float64 restatement against torch float64 autograd of the literal form, the torch float32 goldens
(tests/golden/make_golden_mla.py) against the restatement, the identities the projector obeys, and the presence of the
gdl_mla_* entry points in the header and the binding table."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import mla_ref as mref  # noqa: E402
from gdl import _lib as L  # noqa: E402
from oracle import fixtures as fx  # noqa: E402

GOLD = os.path.join(HERE, "golden")
NAMES = ("gdl_mla_feature_mean", "gdl_mla_projector_update", "gdl_mla_projector_workspace_bytes", "gdl_mla_project",
         "gdl_mla_fuse")


def _feat(seed, B):
    r = np.random.default_rng([73, seed])
    return np.maximum(r.standard_normal((B, 512)), 0).astype(np.float32)


def test_entry_points_declared():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "gdl_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert re.search(r"GDL_API\s+[\w\s\*]+?\b" + n + r"\s*\(", hdr), n
        assert n in L.SIGNATURES, n


def test_schedule_helper():
    import gdl

    assert gdl.mla_alpha(0, 10) == pytest.approx(0.1) and gdl.mla_alpha(10, 10) == pytest.approx(0.01)
    assert gdl.mla_alpha(3, 7) == mref.mla_alpha(3, 7)
    with pytest.raises(ValueError):
        gdl.mla_alpha(0, 0)


@pytest.mark.parametrize("B,n,normalize", [(1, 1, True), (3, 6, True), (5, 34, False), (4, 17, True)])
def test_restatement_against_torch_autograd(B, n, normalize):
    """The literal form: nn.Linear on the features, CrossEntropyLoss, autograd; P as a torch tensor updated as the published
    loop does, weight.grad @ P.T."""
    rng = np.random.default_rng([5, B, n])
    h, rp = _feat(B * 10 + n, B), _feat(99, 7).mean(axis=0)
    W = (0.05 * rng.standard_normal((n, 512))).astype(np.float32)
    b = (0.1 * rng.standard_normal(n)).astype(np.float32)
    lab = rng.integers(0, n, B)
    P0 = mref.projector_update(np.eye(512), _feat(3, 5).mean(axis=0), 0.1, normalize)["P"]
    alpha = 0.0316
    res = mref.half_step_head(h, W, b, lab, P=P0, r_prev=rp, alpha=alpha, normalize=normalize)
    x = torch.from_numpy(h.astype(np.float64)).requires_grad_(True)
    lin = torch.nn.Linear(512, n).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(W.astype(np.float64)))
        lin.bias.copy_(torch.from_numpy(b.astype(np.float64)))
    out = lin(x)
    loss = torch.nn.CrossEntropyLoss()(out, torch.from_numpy(lab))
    loss.backward()
    P = torch.from_numpy(P0.copy())
    r = torch.from_numpy(rp.astype(np.float64))
    k = P @ r
    P = P - torch.outer(k, k) / (float(np.float32(alpha)) + torch.dot(r, k))
    if normalize:
        P = P / torch.norm(P)
    shaped = lin.weight.grad @ P.t()
    np.testing.assert_allclose(res["out"], out.detach().numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(res["loss"], float(loss.detach()), rtol=1e-13)
    np.testing.assert_allclose(res["df"], x.grad.numpy(), rtol=1e-11, atol=1e-17)
    np.testing.assert_allclose(res["dW_plain"], lin.weight.grad.numpy(), rtol=1e-11, atol=1e-17)
    np.testing.assert_allclose(res["db"], lin.bias.grad.numpy(), rtol=1e-11, atol=1e-17)
    np.testing.assert_allclose(res["proj"]["P"], P.numpy(), rtol=1e-12, atol=1e-16)
    np.testing.assert_allclose(res["dW"], shaped.numpy(), rtol=1e-10, atol=1e-17)
    np.testing.assert_allclose(res["r"], x.detach().mean(dim=0).numpy(), rtol=1e-13, atol=1e-18)


@pytest.mark.parametrize("alpha", [0.1, 1e-3])
@pytest.mark.parametrize("normalize", [False, True])
def test_projector_identities(alpha, normalize):
    """P_new r = k alpha / (alpha + r . k) (before the normalisation); the restated P is exactly symmetric; r = 0 leaves P
    unchanged apart from the normalisation."""
    P = np.eye(512)
    for i in range(3):
        r = _feat(i, 6).mean(axis=0)
        res = mref.projector_update(P, r, alpha, normalize)
        a = float(np.float32(alpha))
        # (k - k (r . k) / c cancels down to k alpha / c: the tolerance is float64's on |k|)
        np.testing.assert_allclose(res["P1"] @ res["r"], res["k"] * a / (a + res["r"] @ res["k"]), rtol=1e-9,
                                   atol=1e-13 * np.abs(res["k"]).max())
        assert np.array_equal(res["P"], res["P"].T)
        if normalize:
            assert abs(np.sqrt((res["P"] ** 2).sum()) - 1.0) < 1e-14
        P = res["P"]
    z = mref.projector_update(P, np.zeros(512), alpha, normalize)
    assert np.array_equal(z["P1"], P)
    np.testing.assert_allclose(z["P"], P / np.sqrt((P * P).sum()) if normalize else P, rtol=1e-15)
    b = mref.projector_bounds(res)
    assert np.all(b["P"] > 0) and b["P"].max() < 1e-3  # the bounds are float32-sized on float32-sized data


def test_fusion_restatement():
    rng = np.random.default_rng(11)
    a = rng.standard_normal((6, 9)).astype(np.float32)
    v = (3 * rng.standard_normal((6, 9))).astype(np.float32)
    v[0] = a[0]                       # equal sets: lam exactly 0.5
    v[1] = a[1][::-1]                 # equal entropies from different logits
    a[2] = 0.0
    a[2, 4] = 200.0                   # near one-hot: p = 0 terms contribute 0
    a[3, 1] = np.nan
    out, lam, sa, sv = mref.fuse(a, v, True)
    assert lam[0, 0] == 0.5 and lam[0, 1] == 0.5 and np.array_equal(out[0], a[0].astype(np.float64))
    assert abs(lam[1, 0] - 0.5) < 1e-15 and abs(lam[1, 1] - 0.5) < 1e-15
    assert sa["e"][2] < 1e-80 and np.isfinite(out[2]).all() and lam[2, 0] > lam[2, 1]
    assert np.isnan(lam[3]).all() and np.isnan(out[3]).all() and np.isfinite(out[4:]).all()
    # the literal form in torch float64
    ta, tv = torch.from_numpy(a[4:].astype(np.float64)), torch.from_numpy(v[4:].astype(np.float64))
    ea = -(torch.softmax(ta, 1) * torch.log_softmax(ta, 1)).sum(1)
    ev = -(torch.softmax(tv, 1) * torch.log_softmax(tv, 1)).sum(1)
    w = torch.softmax(torch.stack([-ea, -ev], 1), 1)
    np.testing.assert_allclose(lam[4:], w.numpy(), rtol=1e-12)
    np.testing.assert_allclose(out[4:], (w[:, :1] * ta + w[:, 1:] * tv).numpy(), rtol=1e-12, atol=1e-15)
    o2, l2, _, _ = mref.fuse(a, v, False)
    assert np.all(l2 == 0.5) and np.array_equal(o2[4:], 0.5 * a[4:].astype(np.float64) + 0.5 * v[4:].astype(np.float64))
    b = mref.fuse_bounds(a[4:], v[4:], True)
    assert np.all(b["lam"] > 0) and b["lam"].max() < 1e-4 and b["out"].max() < 1e-3


@pytest.mark.parametrize("name", ["mla_plain_tiny_b4", "mla_gs_tiny_b4"])
def test_goldens_against_restatement(name):
    """What the torch float32 loop recorded against the float64 restatement: the loss and the head's bias gradient from the
    recorded logits, which half-steps were shaped, whose tensors were idle, and P's recorded parts against the projector
    recomputed in float64 from the recorded feature means (the bound is projector_bounds', with torch's unknown summation order
    for the Frobenius norm allowed as gamma over all 512 x 512 terms and the recorded float32 means taken as the inputs)."""
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    cfg = json.loads(str(g["config"]))
    names = [str(n) for n in g["param_names"]]
    assert names[120:] == ["classifier.weight", "classifier.bias"] and len(names) == 122
    P, dP, r_prev = np.eye(512), np.zeros((512, 512)), None
    for st in range(cfg["steps"]):
        _, _, label = fx.make_batch(cfg["seed"] + st, cfg["batch"], cfg["spec_hw"], cfg["frames"], cfg["image_hw"], cfg["n_classes"])
        assert float(g[f"s{st}.a.alpha"]) == mref.mla_alpha(st, cfg["steps_per_epoch"])
        for m in "av":
            pre = f"s{st}.{m}."
            out = g[pre + "out"].astype(np.float64)
            B = out.shape[0]
            mx = out.max(axis=1)
            lse = mx + np.log(np.exp(out - mx[:, None]).sum(axis=1))
            np.testing.assert_allclose(float(g[pre + "loss_f"]), (lse - out[np.arange(B), label]).mean(), rtol=1e-6)
            dl = np.exp(out - lse[:, None])
            dl[np.arange(B), label] -= 1.0
            coef = min(1.0, cfg["max_norm"] / (float(g[pre + "total_norm"]) + 1e-6))
            np.testing.assert_allclose(g[pre + "grad.classifier.bias"], coef * dl.sum(axis=0) / B, rtol=1e-4, atol=1e-6)
            idle = "visual_net." if m == "a" else "audio_net."
            assert [n for n, x in zip(names, g[pre + "grad_is_none"]) if x] == [n for n in names if n.startswith(idle)]
            shaped = cfg["shaping"] and r_prev is not None
            assert int(g[pre + "shaped"]) == int(shaped)
            if shaped:
                res = mref.projector_update(P, r_prev, float(g[pre + "alpha"]), True)
                S = res["norm"] ** 2
                b = mref.projector_bounds(res, dP=dP)["P"] + np.abs(res["P"]) * mref.gamma(512 * 512) / 2
                P, dP = res["P"], b
                assert S > 0
            want = mref.p_summary(P)
            bound = dP  # (zero until the first shaped half-step: P is the identity, recorded exactly)
            assert np.all(np.abs(g[pre + "P16"] - want["P16"]) <= bound[:16, :16] + 1e-30), pre
            assert np.all(np.abs(g[pre + "Pdiag"] - want["Pdiag"]) <= np.diag(bound) + 1e-30), pre
            assert np.all(np.abs(g[pre + "Prowsum"] - want["Prowsum"]) <= bound.sum(axis=1) + 1e-30), pre
            assert abs(float(g[pre + "Pfro"]) - want["Pfro"]) <= np.sqrt((bound * bound).sum()) + 1e-30, pre
            r_prev = g[pre + "r"].astype(np.float64)
    if not cfg["shaping"]:
        assert float(g["s1.v.Pfro"]) == np.sqrt(512.0) and np.all(g["s1.v.Pdiag"] == 1.0)
