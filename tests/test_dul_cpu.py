"""CPU tests of the probabilistic-embedding branch (main.py --pe 1 --beta b): tests/dul_ref.py, the float64 yardstick of the GPU
tests, against torch float64 autograd of the literal form -- nn.Conv2d(512, 512, 1) + nn.BatchNorm2d(512) twice, exp(0.5 lv), a
supplied eps, AdaptiveAvgPool2d, `regurize` as main.py:92-102 writes it -- the pooled eval form against the literal order, the
named departure db_conv = 0, the generator's keying, and the module side of the switch (names, order, checkpoints)."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dul_ref as dr  # noqa: E402
import modulation_ref as mr  # noqa: E402

DUL_NAMES = list(dr.DUL_NAMES)


def regurize(mul, std):
    """main.py:92-102"""
    variance_dul = (std ** 2).view(std.shape[0], -1)
    mul = mul.view(mul.shape[0], -1)
    loss_kl = (variance_dul + mul ** 2 - torch.log(variance_dul + 1e-8) - 1) * 0.5
    return torch.mean(torch.sum(loss_kl, dim=1))


def _case(n_img, T, h, w, seed):
    rng = np.random.default_rng(seed)
    P_ = h * w
    x = np.maximum(rng.standard_normal((n_img, 512, h, w)), 0.0)  # a post-ReLU map, NCHW
    P = [rng.standard_normal((512, 512, 1, 1)) * 0.05, rng.standard_normal(512) * 0.1, 1 + 0.1 * rng.standard_normal(512),
         0.1 * rng.standard_normal(512), rng.standard_normal((512, 512, 1, 1)) * 0.05, rng.standard_normal(512) * 0.1,
         1 + 0.1 * rng.standard_normal(512), 0.1 * rng.standard_normal(512)]
    eps = rng.standard_normal((n_img, 512, h, w))
    r = rng.standard_normal((n_img // T, 512))
    return x, P, eps, r, P_


def _literal(x, P, eps, r, T, beta, train=True):
    """the literal form in torch float64: (stacks, x leaf, f, reg, mu, sd)"""
    stacks = []
    for i in (0, 4):
        s = nn.Sequential(nn.Conv2d(512, 512, kernel_size=1, stride=1, padding=0), nn.BatchNorm2d(512)).double()
        with torch.no_grad():
            for p, v in zip(s.parameters(), P[i:i + 4]):
                p.copy_(torch.from_numpy(np.asarray(v)))
        stacks.append(s.train(train))
    xt = torch.from_numpy(x).requires_grad_(True)
    mu, lv = stacks[0](xt), stacks[1](xt)
    sd = (lv * 0.5).exp()
    out = mu + torch.from_numpy(eps) * sd if train else mu
    n_img = x.shape[0]
    f = nn.AdaptiveAvgPool2d(1)(out).flatten(1)  # [n_img, 512]
    f = f.view(n_img // T, T, 512).mean(1)       # basic_model.py:73-82 for equal-sized frames
    reg = regurize(mu, sd)
    return stacks, xt, f, reg, mu, sd


def _rows(a):  # NCHW -> [M][512]
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1))).reshape(-1, 512)


@pytest.mark.parametrize("n_img,T,h,w,beta", [(4, 1, 2, 3, 1e-2), (6, 3, 2, 2, 1e-5), (6, 3, 2, 2, 0.0)])
def test_ref_matches_torch_float64_autograd(n_img, T, h, w, beta):
    x, P, eps, r, P_ = _case(n_img, T, h, w, 1)
    stacks, xt, f, reg, mu, sd = _literal(x, P, eps, r, T, beta)
    loss = (f * torch.from_numpy(r)).sum() + beta * reg
    loss.backward()
    ref = dr.stage(_rows(x), P, _rows(eps), lambda f_: r, beta, n_img, T)
    tol = dict(rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(ref["f"], f.detach().numpy(), **tol)
    np.testing.assert_allclose(ref["reg"], reg.item(), **tol)
    np.testing.assert_allclose(ref["mu"], _rows(mu.detach().numpy()), **tol)
    np.testing.assert_allclose(ref["sd"], _rows(sd.detach().numpy()), **tol)
    got = [p.grad.numpy() for s in stacks for p in s.parameters()]
    for i, (name, g, e) in enumerate(zip(DUL_NAMES, got, ref["dP"])):
        if i in (1, 5):  # db_conv: the named departure, below
            continue
        np.testing.assert_allclose(e, g, rtol=1e-8, atol=1e-12 * max(1.0, np.abs(g).max()), err_msg=name)
    np.testing.assert_allclose(ref["dx"], _rows(xt.grad.numpy()), rtol=1e-8, atol=1e-12)
    # running statistics: the bias is part of the batch mean; the unbiased variance with momentum 0.1
    M = n_img * P_
    for s, bn, var in ((stacks[0], ref["bn_mu"], ref["var_mu"]), (stacks[1], ref["bn_lv"], ref["var_lv"])):
        rm, rv = dr.running_update(np.zeros(512), np.ones(512), bn[2], var, M)
        np.testing.assert_allclose(rm, s[1].running_mean.numpy(), **tol)
        np.testing.assert_allclose(rv, s[1].running_var.numpy(), **tol)
        assert int(s[1].num_batches_tracked) == 1


def test_conv_bias_gradient_is_rounding_noise():
    """db_conv = sum over rows of dz, which is 0 in real arithmetic: sum_r (d - mean(d) - xhat mean(d xhat)) = 0 because
    sum xhat = 0.  torch leaves the float64 rounding of that sum.  Bound: every dz term g (d - c0 - xhat c1), g = gamma rstd,
    carries at most 8 roundings of magnitude at most A = |g| (|d| + |c0| + |xhat c1|) (the means' own errors included: they
    are sums of M terms accumulated pairwise, <= log2(M) + 1 roundings, taken as M to be safe), and the M-term sum adds
    M roundings of the partial sums, each at most sum A: |db| <= (8 + 2 M) 2^-53 sum_rows A."""
    n_img, T, h, w, beta = 6, 3, 2, 2, 1e-2
    x, P, eps, r, P_ = _case(n_img, T, h, w, 2)
    stacks, xt, f, reg, mu, sd = _literal(x, P, eps, r, T, beta)
    ((f * torch.from_numpy(r)).sum() + beta * reg).backward()
    ref = dr.stage(_rows(x), P, _rows(eps), lambda f_: r, beta, n_img, T)
    M = n_img * P_
    d_mu, d_lv = dr.grads(ref, r, _rows(eps), beta, n_img, T)
    for s, d, z, bn, gamma, e in ((stacks[0], d_mu, ref["z_mu"], ref["bn_mu"], P[2], ref["dP"][1]),
                                  (stacks[1], d_lv, ref["z_lv"], ref["bn_lv"], P[6], ref["dP"][5])):
        b = dr.bn_backward(d, z, bn, gamma)
        A = np.abs(gamma * bn[3]) * (np.abs(d) + np.abs(b["coef"][0]) + np.abs(b["xhat"] * b["coef"][1]))
        bound = (8 + 2 * M) * 2.0 ** -53 * A.sum(0)
        db = s[0].bias.grad.numpy()
        assert np.all(np.abs(db) <= bound), float((np.abs(db) / bound).max())
        assert np.all(e == 0.0)  # the departure: exactly zero
        assert np.abs(db).max() < 1e-6 * np.abs(s[0].weight.grad.numpy()).max()


def test_eval_form_matches_literal_order():
    """eval: out = mu with running statistics, then the pool -- against pool first, then one 512 x 512 product per sample"""
    n_img, T, h, w = 6, 3, 2, 3
    x, P, eps, r, P_ = _case(n_img, T, h, w, 3)
    rng = np.random.default_rng(4)
    rm, rv = rng.standard_normal(512) * 0.2, 0.5 + rng.random(512)
    stacks, xt, f, reg, mu, sd = _literal(x, P, eps, r, T, 0.0, train=True)  # (build), then set the buffers and re-run in eval
    with torch.no_grad():
        stacks[0][1].running_mean.copy_(torch.from_numpy(rm))
        stacks[0][1].running_var.copy_(torch.from_numpy(rv))
        stacks[0].eval()
        out = stacks[0](torch.from_numpy(x))
        lit = nn.AdaptiveAvgPool2d(1)(out).flatten(1).view(n_img // T, T, 512).mean(1).numpy()
    pooled = _rows(x).reshape(n_img // T, T * P_, 512).mean(1)
    sc, sh = dr.eval_scale_shift(P[2], P[3], rm, rv)
    np.testing.assert_allclose(dr.eval_form(pooled, P[0], P[1], sc, sh), lit, rtol=1e-10, atol=1e-12)


def test_generator_keying():
    """the normals are those of the modulation's generator on a disjoint counter range: word 1 = 0x80000000 | modality"""
    z = dr.normals(4096, seed=7, step=3, modality=dr.AUDIO)
    assert abs(z.mean()) < 0.06 and abs(z.std() - 1) < 0.05
    q = np.arange(1024, dtype=np.int64)
    w = mr.philox4x32_10((q, np.full_like(q, 0x80000000), np.full_like(q, 3), np.zeros_like(q)), (7, 0))
    z0, z1 = mr.box_muller(w[0], w[1])
    z2, z3 = mr.box_muller(w[2], w[3])
    assert np.array_equal(z.reshape(-1, 4), np.stack([z0, z1, z2, z3], 1))
    # the streams differ: modality, step, seed -- and from the modulation's stream of the same (seed, step)
    assert not np.allclose(z, dr.normals(4096, 7, 3, dr.VISUAL))
    assert not np.allclose(z, dr.normals(4096, 7, 4, dr.AUDIO))
    assert not np.allclose(z, dr.normals(4096, 8, 3, dr.AUDIO))
    assert not np.allclose(z, mr.normals(np.arange(4096, dtype=np.int64), 7, 3))
    # a prefix of a longer map is the shorter map: a function of the element index alone
    assert np.array_equal(z[:100], dr.normals(100, 7, 3, dr.AUDIO))


# ------------------------------------------------------------------------------------------------------------ the module side
def _args(**kw):
    return argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=4, **kw)


def test_module_parameter_names_and_order_with_pe():
    from models.backbone import resnet18

    for modality in ("audio", "visual"):
        off = resnet18(modality, _args())
        on = resnet18(modality, _args(pe=1))
        names_off = [n for n, _ in off.named_parameters()]
        names_on = [n for n, _ in on.named_parameters()]
        assert len(names_off) == 60
        assert names_on == names_off + DUL_NAMES
        shapes = [tuple(p.shape) for _, p in on.named_parameters()][60:]
        assert shapes == [(512, 512, 1, 1), (512,), (512,), (512,)] * 2
        extra = [k for k in on.state_dict() if k not in off.state_dict()]
        assert extra == DUL_NAMES[:4] + ["mu_dul_backbone.1.running_mean", "mu_dul_backbone.1.running_var",
                                         "mu_dul_backbone.1.num_batches_tracked"] + DUL_NAMES[4:] + \
            ["logvar_dul_backbone.1.running_mean", "logvar_dul_backbone.1.running_var", "logvar_dul_backbone.1.num_batches_tracked"]
        assert [id(p) for p in on.engine_parameters()] == [id(p) for p in list(on.parameters())[:60]]
        assert [id(p) for p in on.dul_parameters()] == [id(p) for p in list(on.parameters())[60:]]
        assert len(off.engine_parameters()) == 60


def test_module_unchanged_with_pe_off():
    """pe absent, pe = 0: the same parameters, the same state_dict keys, the same seeded initial values"""
    from models.basic_model import AVClassifier, AVClassifier_DGL

    for cls in (AVClassifier, AVClassifier_DGL):
        torch.manual_seed(0)
        a = cls(_args())
        torch.manual_seed(0)
        b = cls(_args(pe=0))
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        assert list(a.state_dict()) == list(b.state_dict())
        assert not any("_dul_" in k for k in a.state_dict())
        for (k, u), v in zip(a.state_dict().items(), b.state_dict().values()):
            assert torch.equal(u, v), k


def test_models_pass_pe_through_and_checkpoint_round_trips():
    from models.basic_model import AVClassifier, AVClassifier_DGL
    from utils.utils import weight_init

    for cls, modality in ((AVClassifier, "full"), (AVClassifier_DGL, "full"), (AVClassifier_DGL, "audio"), (AVClassifier_DGL, "visual")):
        args = _args(pe=1)
        args.modality = modality
        m = cls(args)
        nets = [n for n in ("audio_net", "visual_net") if hasattr(m, n) and getattr(m, n) is not None]
        assert nets
        keys = list(m.state_dict())
        for n in nets:
            for k in DUL_NAMES:
                assert f"{n}.{k}" in keys
        m.apply(weight_init)  # Conv2d: Kaiming normal; BatchNorm2d: gamma 1, beta 0 -- like any other
        net = getattr(m, nets[0])
        assert torch.all(net.mu_dul_backbone[1].weight == 1) and torch.all(net.logvar_dul_backbone[1].bias == 0)
        assert float(net.mu_dul_backbone[0].weight.detach().std()) > 0
        m2 = cls(args)
        m2.load_state_dict(m.state_dict(), strict=True)
        for (k, u), v in zip(m.state_dict().items(), m2.state_dict().values()):
            assert torch.equal(u, v), k
        # a checkpoint without the branch does not load into a model with it, and the reverse
        args0 = _args()
        args0.modality = modality
        with pytest.raises(RuntimeError):
            m.load_state_dict(cls(args0).state_dict(), strict=True)
        with pytest.raises(RuntimeError):
            cls(args0).load_state_dict(m.state_dict(), strict=True)


def test_module_forward_with_pe_names_the_native_runners():
    from models.backbone import resnet18

    net = resnet18("audio", _args(pe=1))
    with pytest.raises(NotImplementedError, match="UnimodalTrainer"):
        net(torch.zeros(2, 1, 65, 47))
