"""GPU tests of the probabilistic-embedding branch (main.py --pe 1 --beta b): the four kernels of csrc/dul.hip through the C ABI
on free-standing maps against the float64 restatement of tests/dul_ref.py with its derived bounds (pinned on the CPU by
tests/test_dul_cpu.py), the generator's keying, the argument checks, and the runners --
UnimodalTrainer and DGLTrainer with the branch -- against the literal torch step goldens of tests/golden/make_golden_dul.py,
run to run, across a checkpoint, with the switch off, in valid() and in every refusal."""
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

import dul_ref as dr  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev  # noqa: E402

from oracle import fixtures as fx  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = [L.GDL_F32, L.GDL_BF16]
# (n_img, T, P): M = 18 under one tile; samples of several images (the pool crosses image boundaries, KL divisor 12 not 4);
# one sample of 54 rows; M = 3 456 -- several blocks of every kernel, the second-stage fold of the KL sum
SHAPES = [(3, 1, 6), (12, 3, 4), (2, 1, 54), (64, 1, 54)]
SEED, STEP = 0x1234567855, 7


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _maps(n_img, T, P, dt, seed=0):
    """z_mu, z_lv [M][512] in the storage dtype and the two stacks' constants bn = [4][512] (scale, shift, mean, rstd)"""
    rng = np.random.default_rng(seed + 1000 * n_img + P)
    M = n_img * P
    td = L.torch_dtype(dt)
    z_mu = dev(rng.standard_normal((M, 512)) * 1.5 + 0.3, td)
    z_lv = dev(rng.standard_normal((M, 512)) * 1.2 - 0.2, td)
    bn = []
    for _ in range(2):
        rstd = 0.5 + rng.random(512)
        gamma = 1 + 0.2 * rng.standard_normal(512)
        mean = 0.3 * rng.standard_normal(512)
        bn.append(np.stack([gamma * rstd, 0.1 * rng.standard_normal(512) - mean * gamma * rstd, mean, rstd]).astype(np.float32))
    gam = [(b[0] / b[3]).astype(np.float32) for b in bn]
    return z_mu, z_lv, dev(bn[0]), dev(bn[1]), dev(gam[0]), dev(gam[1])


def _ws(dt, n_img, T):
    nb = L.load().gdl_dul_sample_workspace_bytes(dt, n_img, T)
    assert nb >= 256 + 4
    return torch.zeros(nb, dtype=torch.uint8, device=DEV), nb


def _sample(dt, z_mu, z_lv, bn_mu, bn_lv, n_img, T, P, eps_in=None, maps=True, modality=L.GDL_AUDIO, seed=SEED, step=STEP, ws=None):
    M = n_img * P
    f = torch.full((n_img // T, 512), float("nan"), device=DEV)
    reg = torch.full((1,), float("nan"), device=DEV)
    mm = [torch.full((M, 512), float("nan"), device=DEV) for _ in range(4)] if maps else [None] * 4
    ws, nb = ws if ws is not None else _ws(dt, n_img, T)
    L.call("gdl_dul_sample", dt, L.ptr(z_mu), L.ptr(z_lv), L.ptr(bn_mu), L.ptr(bn_lv), L.ptr(eps_in), seed, step, modality, L.ptr(f),
           L.ptr(reg), L.ptr(mm[0]), L.ptr(mm[1]), L.ptr(mm[2]), L.ptr(mm[3]), n_img, T, P, 512, L.ptr(ws), nb, L.cur_stream())
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32)[0]) == 0  # the ticket counter is handed back at zero
    return f, reg, mm


def _np64(t):
    return t.double().cpu().numpy()


def _within(got, want, bound, what):
    err = np.abs(_np64(got) - want)
    floor = 1e-37  # (results in the subnormal range)
    bad = err > bound + floor
    assert not bad.any(), (what, float((err / (bound + floor)).max()), int(bad.sum()))
    return float((err / (bound + floor)).max())


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_sample_against_ref(shape, dt):
    n_img, T, P = shape
    z_mu, z_lv, bn_mu, bn_lv, _, _ = _maps(n_img, T, P, dt)
    f, reg, (mu, sd, eps, out) = _sample(dt, z_mu, z_lv, bn_mu, bn_lv, n_img, T, P)
    # the noise: the reference's normals (1e-3: the bound tests/test_modulation_gpu.py holds these normals to -- float32 sincos and
    # the rounding of the radius; a wrong counter word or lane is off by O(1))
    want_eps = dr.normals(n_img * P * 512, SEED, STEP, dr.AUDIO).reshape(-1, 512)
    assert np.abs(_np64(eps) - want_eps).max() < 1e-3
    r = dr.sample(_np64(z_mu), _np64(z_lv), _np64(bn_mu), _np64(bn_lv), _np64(eps), n_img, T)
    e_mu, e_sd, e_out, e_f, e_reg = dr.sample_bounds(r, _np64(eps), n_img, T, 2 if dt == L.GDL_BF16 else 4)
    worst = {k: _within(g, r[k], e, k) for k, g, e in (("mu", mu, e_mu), ("sd", sd, e_sd), ("out", out, e_out), ("f", f, e_f))}
    worst["reg"] = _within(reg, np.array([r["reg"]]), np.array([e_reg]), "reg")
    print(f"dul sample {shape} dt={dt}: error / bound {worst}")
    # without the optional maps (the training step's call): the same f and reg, bit for bit; and run to run
    f2, reg2, _ = _sample(dt, z_mu, z_lv, bn_mu, bn_lv, n_img, T, P, maps=False)
    assert _same_bits(f, f2) and _same_bits(reg, reg2)


def test_noise_streams_differ():
    n_img, T, P = 3, 1, 6
    z_mu, z_lv, bn_mu, bn_lv, _, _ = _maps(n_img, T, P, L.GDL_F32)
    base = _sample(L.GDL_F32, z_mu, z_lv, bn_mu, bn_lv, n_img, T, P)[2][2]
    for kw, ref in ((dict(modality=L.GDL_VISUAL), dr.normals(18 * 512, SEED, STEP, dr.VISUAL)),
                    (dict(step=STEP + 1), dr.normals(18 * 512, SEED, STEP + 1, dr.AUDIO)),
                    (dict(seed=SEED + 1), dr.normals(18 * 512, SEED + 1, STEP, dr.AUDIO)),
                    (dict(step=STEP + (1 << 32)), dr.normals(18 * 512, SEED, STEP + (1 << 32), dr.AUDIO))):
        other = _sample(L.GDL_F32, z_mu, z_lv, bn_mu, bn_lv, n_img, T, P, **kw)[2][2]
        assert float((other - base).abs().mean()) > 0.5  # independent normals: E|a - b| = 2 / sqrt(pi) = 1.13
        assert np.abs(_np64(other).reshape(-1) - ref).max() < 1e-3


@pytest.mark.parametrize("dt", DTYPES)
def test_supplied_eps_is_used_bit_for_bit(dt):
    n_img, T, P = 12, 3, 4
    z_mu, z_lv, bn_mu, bn_lv, _, _ = _maps(n_img, T, P, dt)
    eps_in = torch.randn(n_img * P, 512, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    f, reg, (mu, sd, eps, out) = _sample(dt, z_mu, z_lv, bn_mu, bn_lv, n_img, T, P, eps_in=eps_in)
    assert _same_bits(eps, eps_in)
    # out = fmaf(eps, sd, mu) of the returned maps: the product of two float32 is exact in the 64-bit significand of long double
    ld = lambda t: t.cpu().numpy().astype(np.longdouble)  # noqa: E731
    want = (ld(eps) * ld(sd) + ld(mu)).astype(np.float32)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ backward
def _backward(dt, z_mu, z_lv, bn_mu, bn_lv, gam_mu, gam_lv, df, eps_in, beta, n_img, T, P, modality=L.GDL_AUDIO):
    lib = L.load()
    M = n_img * P
    blocks = lib.gdl_bn_bwd_blocks(M, 512)
    part = [torch.full((blocks, 512, 2), float("nan"), device=DEV) for _ in range(2)]
    st = L.cur_stream()
    L.call("gdl_dul_bwd_reduce", dt, L.ptr(z_mu), L.ptr(z_lv), L.ptr(df), L.ptr(eps_in), SEED, STEP, modality, beta, L.ptr(bn_mu),
           L.ptr(bn_lv), L.ptr(part[0]), L.ptr(part[1]), n_img, T, P, 512, st)
    dgam, dbet, coef = ([torch.empty(512, device=DEV) for _ in range(2)], [torch.empty(512, device=DEV) for _ in range(2)],
                        [torch.empty(2, 512, device=DEV) for _ in range(2)])
    for i in range(2):
        L.call("gdl_bn_bwd_finalize", L.ptr(part[i]), blocks, 512, float(M), L.ptr(dgam[i]), L.ptr(dbet[i]), L.ptr(coef[i]), st)
    dz = [torch.full((M, 512), float("nan"), device=DEV, dtype=L.torch_dtype(dt)) for _ in range(2)]
    L.call("gdl_dul_bwd_apply", dt, L.ptr(z_mu), L.ptr(z_lv), L.ptr(df), L.ptr(eps_in), SEED, STEP, modality, beta, L.ptr(bn_mu),
           L.ptr(bn_lv), L.ptr(gam_mu), L.ptr(gam_lv), L.ptr(coef[0]), L.ptr(coef[1]), L.ptr(dz[0]), L.ptr(dz[1]), n_img, T, P, 512, st)
    torch.cuda.synchronize()
    return part, dgam, dbet, coef, dz, blocks


@pytest.mark.parametrize("beta", [0.0, 1e-2])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_ref(shape, dt, beta):
    n_img, T, P = shape
    M = n_img * P
    z_mu, z_lv, bn_mu, bn_lv, gam_mu, gam_lv = _maps(n_img, T, P, dt)
    eps = _sample(dt, z_mu, z_lv, bn_mu, bn_lv, n_img, T, P)[2][2]  # the forward's own noise
    df = torch.randn(n_img // T, 512, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    part, dgam, dbet, coef, dz, blocks = _backward(dt, z_mu, z_lv, bn_mu, bn_lv, gam_mu, gam_lv, df, eps, beta, n_img, T, P)
    # float32(beta), as the ABI passes it; the reference divides it by n_img in double (2 u |k| in the bounds)
    b32 = float(np.float32(beta))
    r = dr.sample(_np64(z_mu), _np64(z_lv), _np64(bn_mu), _np64(bn_lv), _np64(eps), n_img, T)
    d = dr.grads(r, _np64(df), _np64(eps), b32, n_img, T)
    e_d = dr.grad_bounds(r, _np64(df), _np64(eps), b32, n_img, T)
    eb = 2 if dt == L.GDL_BF16 else 4
    rows = -(-(M * 512 // (16 // eb)) // (blocks * 256))
    worst = {}
    for i, (z, bn, gam) in enumerate(((z_mu, bn_mu, gam_mu), (z_lv, bn_lv, gam_lv))):
        b = dr.bn_backward(d[i], _np64(z), _np64(bn), _np64(gam))
        e_S1, e_S2, e_dz = dr.bn_backward_bounds(b, d[i], e_d[i], _np64(bn), _np64(gam), rows, eb)
        tag = "mu" if i == 0 else "lv"
        # the channel sums: the per-block partials added in double = what gdl_bn_bwd_finalize leaves as dbeta / dgamma
        worst["S1_" + tag] = _within(part[i][:, :, 0].double().sum(0), b["S1"], e_S1, "S1 " + tag)
        worst["S2_" + tag] = _within(part[i][:, :, 1].double().sum(0), b["S2"], e_S2, "S2 " + tag)
        worst["dbeta_" + tag] = _within(dbet[i], b["S1"], e_S1, "dbeta " + tag)
        worst["dgamma_" + tag] = _within(dgam[i], b["S2"], e_S2, "dgamma " + tag)
        worst["dz_" + tag] = _within(dz[i], b["dz"], e_dz, "dz " + tag)
    print(f"dul backward {shape} dt={dt} beta={beta}: error / bound {worst}")
    # the backward that regenerates the noise gives the same bytes as the one fed the forward's eps map
    part2, dgam2, dbet2, coef2, dz2, _ = _backward(dt, z_mu, z_lv, bn_mu, bn_lv, gam_mu, gam_lv, df, None, beta, n_img, T, P)
    for a, b_ in zip(part + dgam + dbet + coef, part2 + dgam2 + dbet2 + coef2):
        assert _same_bits(a, b_)
    for a, b_ in zip(dz, dz2):
        assert torch.equal(a.view(torch.int16 if dt == L.GDL_BF16 else torch.int32), b_.view(torch.int16 if dt == L.GDL_BF16 else torch.int32))


# ------------------------------------------------------------------------------------------------------------------ eval
@pytest.mark.parametrize("B", [2, 64])
def test_eval_against_ref(B):
    rng = np.random.default_rng(B)
    f = dev(np.abs(rng.standard_normal((B, 512))))
    W = dev(rng.standard_normal((512, 512)) * 0.05)
    b = dev(rng.standard_normal(512) * 0.1)
    gamma, beta = dev(1 + 0.1 * rng.standard_normal(512)), dev(0.1 * rng.standard_normal(512))
    rm, rv = dev(0.2 * rng.standard_normal(512)), dev(0.5 + rng.random(512))
    sc, sh = torch.empty(512, device=DEV), torch.empty(512, device=DEV)
    out = torch.full((B, 512), float("nan"), device=DEV)
    st = L.cur_stream()
    L.call("gdl_bn_finalize_eval", 512, L.ptr(gamma), L.ptr(beta), 1e-5, L.ptr(rm), L.ptr(rv), L.ptr(sc), L.ptr(sh), st)
    L.call("gdl_dul_eval", L.ptr(f), L.ptr(W), L.ptr(b), L.ptr(sc), L.ptr(sh), L.ptr(out), B, 512, st)
    torch.cuda.synchronize()
    a = [_np64(t) for t in (f, W, b, sc, sh)]
    _within(out, dr.eval_form(*a), dr.eval_bound(*a), "eval")
    # ... and the whole eval form from the running statistics: gdl_bn_finalize_eval works in double and rounds scale and shift to
    # float32 once each, u |scale|, u |shift| with |shift| <= |beta| + |rm scale|; the slack below is 8 times that
    sc64, sh64 = dr.eval_scale_shift(_np64(gamma), _np64(beta), _np64(rm), _np64(rv))
    want = dr.eval_form(a[0], a[1], a[2], sc64, sh64)
    dot_b = np.abs(a[0] @ a[1].T + a[2])
    slack = 4 * dr.U * (dot_b * np.abs(sc64) + np.abs(_np64(rm) * sc64) + np.abs(_np64(beta)))
    _within(out, want, dr.eval_bound(a[0], a[1], a[2], sc64, sh64) + 2 * slack, "eval from running statistics")


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_return_without_a_launch():
    lib = L.load()
    n_img, T, P, dt = 3, 1, 6, L.GDL_F32
    M = n_img * P
    z_mu, z_lv, bn_mu, bn_lv, gam_mu, gam_lv = _maps(n_img, T, P, dt)
    f, reg = torch.full((n_img, 512), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
    ws, nb = _ws(dt, n_img, T)
    st = L.cur_stream()
    good = dict(dt=dt, z_mu=L.ptr(z_mu), z_lv=L.ptr(z_lv), bn_mu=L.ptr(bn_mu), bn_lv=L.ptr(bn_lv), eps=None, f=L.ptr(f), reg=L.ptr(reg),
                n_img=n_img, T=T, P=P, C=512, ws=L.ptr(ws), nb=nb, modality=0)

    def sample(**kw):
        a = {**good, **kw}
        return lib.gdl_dul_sample(a["dt"], a["z_mu"], a["z_lv"], a["bn_mu"], a["bn_lv"], a["eps"], SEED, STEP, a["modality"], a["f"],
                                  a["reg"], None, None, None, None, a["n_img"], a["T"], a["P"], a["C"], a["ws"], a["nb"], st)

    bad = [dict(C=256), dict(C=1024), dict(P=0), dict(T=0), dict(n_img=0), dict(T=2), dict(dt=5), dict(modality=2), dict(z_mu=None),
           dict(z_lv=None), dict(bn_mu=None), dict(f=None), dict(reg=None), dict(ws=None), dict(z_mu=L.ptr(z_mu) + 4),
           dict(bn_lv=L.ptr(bn_lv) + 4), dict(eps=L.ptr(z_mu) + 8), dict(ws=L.ptr(ws) + 64), dict(nb=nb - 1), dict(nb=0)]
    for kw in bad:
        assert sample(**kw) == 1, kw  # GDL_ERR_ARG
        assert L.last_error().startswith("dul_sample"), (kw, L.last_error())
    df = torch.randn(n_img, 512, device=DEV)
    blocks = lib.gdl_bn_bwd_blocks(M, 512)
    part = [torch.full((blocks, 512, 2), 7.0, device=DEV) for _ in range(2)]
    coef = torch.zeros(2, 512, device=DEV)
    dz = [torch.full((M, 512), 7.0, device=DEV) for _ in range(2)]

    def reduce_(z=L.ptr(z_mu), d=L.ptr(df), p=L.ptr(part[0]), C=512, T_=T, P_=P):
        return lib.gdl_dul_bwd_reduce(dt, z, L.ptr(z_lv), d, None, SEED, STEP, 0, 0.0, L.ptr(bn_mu), L.ptr(bn_lv), p, L.ptr(part[1]),
                                      n_img, T_, P_, C, st)

    def apply_(z=L.ptr(z_mu), c=L.ptr(coef), o=L.ptr(dz[0]), C=512, T_=T, P_=P):
        return lib.gdl_dul_bwd_apply(dt, z, L.ptr(z_lv), L.ptr(df), None, SEED, STEP, 0, 0.0, L.ptr(bn_mu), L.ptr(bn_lv), L.ptr(gam_mu),
                                     L.ptr(gam_lv), c, L.ptr(coef), o, L.ptr(dz[1]), n_img, T_, P_, C, st)

    for fn in (reduce_, apply_):
        for kw in (dict(C=64), dict(T_=0), dict(P_=0), dict(T_=2), dict(z=None), dict(z=L.ptr(z_mu) + 4)):
            assert fn(**kw) == 1, (fn.__name__, kw)
    assert reduce_(d=None) == 1 and reduce_(p=None) == 1 and reduce_(p=L.ptr(part[0]) + 4) == 1
    assert apply_(c=None) == 1 and apply_(o=None) == 1 and apply_(o=L.ptr(dz[0]) + 8) == 1
    out = torch.full((2, 512), 7.0, device=DEV)
    W = torch.zeros(512, 512, device=DEV)

    def eval_(f_=L.ptr(df), w=L.ptr(W), o=L.ptr(out), B=2, C=512):
        return lib.gdl_dul_eval(f_, w, L.ptr(gam_mu), L.ptr(gam_mu), L.ptr(gam_mu), o, B, C, st)

    for kw in (dict(C=256), dict(B=0), dict(f_=None), dict(w=None), dict(o=None), dict(o=L.ptr(df)), dict(f_=L.ptr(df) + 2)):
        assert eval_(**kw) == 1, kw
    assert lib.gdl_dul_sample_workspace_bytes(7, 3, 1) == 0 and lib.gdl_dul_sample_workspace_bytes(dt, 0, 1) == 0
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill, the ticket counter is untouched
    for t in [f, reg, out] + part + dz:
        assert bool((t == 7.0).all())
    assert int(ws.view(torch.int32)[0]) == 0
    assert sample() == 0  # (the accepted call, for contrast)
    torch.cuda.synchronize()
    assert not bool((f == 7.0).any())


# ================================================================================================================== the runners
def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def _pe_model(kind, fusion, dtype, pe=1, with_pe_attr=True):
    """the mirror model of a golden configuration on the device, the fixtures' state loaded by name"""
    from models.basic_model import AVClassifier, AVClassifier_DGL

    args = argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality="audio" if kind == "unimodal" else "full", batch_size=4)
    if with_pe_attr:
        args.pe = pe
    model = (AVClassifier if kind == "joint" else AVClassifier_DGL)(args)
    ps, bs = fx.model_state(6, fusion + "_dgl" if kind != "joint" else "concat")
    sd = {**ps, **bs}
    if kind == "unimodal":
        sd = {k: v for k, v in sd.items() if k.startswith(("fusion_module.", "audio_net."))}
        sd.update(fx.make_state({"audio_classifier.weight": (6, 512), "audio_classifier.bias": (6,)}))
    if pe and with_pe_attr:
        for pre in ("audio_net.",) + (() if kind == "unimodal" else ("visual_net.",)):
            dp, db = dr.dul_state(pre)
            sd.update(dp)
            sd.update(db)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    model = model.to(DEV)
    for n in ("audio_net", "visual_net"):
        if getattr(model, n, None) is not None:
            getattr(model, n).gdl_dtype = dtype
    return model.train()


def _pe_trainer(kind, fusion, dtype, beta, seed=0, **kw):
    from gdl.trainer import DGLTrainer
    from gdl.unimodal import UnimodalTrainer

    model = _pe_model(kind, fusion, dtype, **kw)
    if kind == "unimodal":
        return model, UnimodalTrainer(model, lr=2e-3, beta=beta, seed=seed)
    if kind == "joint":
        return model, DGLTrainer(model, lr=2e-3, mode="joint", beta=beta, seed=seed)
    return model, DGLTrainer(model, lr=2e-3, alpha=2.5, mode="dgl", detach_fused=False, drop_head_uni=False, beta=beta, seed=seed)


def _gbatch(cfg, st):
    spec, image, label = fx.make_batch(cfg["seed"] + st, cfg["batch"], cfg["spec_hw"], cfg["frames"], cfg["image_hw"], cfg["n_classes"])
    return dev(spec), dev(image), torch.from_numpy(label).to(DEV)


def _geps(cfg, st):
    """the goldens' injected noise as `pe_eps`: audio map 3 x 2 positions per image, visual 2 x 2 per frame"""
    B, T = cfg["batch"], cfg["frames"]
    return (dev(dr.golden_eps(B, 6, cfg["eps_seed"], st, dr.AUDIO)), dev(dr.golden_eps(B * T, 4, cfg["eps_seed"], st, dr.VISUAL)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["dul_uni_audio_tiny_b4", "dul_joint_concat_tiny_b4", "dul_joint_concat_beta2_tiny_b4", "dul_mtl_sum_tiny_b4"])
def test_trainer_step_golden(name, dtype):
    """The runners with the branch against the literal torch float32 step (tests/golden/make_golden_dul.py) with its noise supplied
    as `pe_eps`, to the constants tests/test_joint_gpu.py::test_joint_step_golden and tests/test_unimodal_gpu.py hold their own
    step goldens to in the same dtype: float32 first step logits / loss 5e-4, total norm 3e-3, grad sums 6e-3, per-tensor norms
    1e-2 (later steps 1e-2, 2e-2, 4e-2, 6e-2); bf16 first step 0.2, 5e-2, 4e-2, 8e-2, 0.3, later steps finite.  The regulariser:
    the logits' relative bound (it is a mean of O(1) terms of the same maps)."""
    g = _gold(name)
    cfg = json.loads(str(g["config"]))
    kind = cfg["mode"]
    model, tr = _pe_trainer(kind, cfg["fusion"], dtype, cfg["beta"])
    ne = 68
    assert len(tr.names) == tr.nf + ne * (1 if kind == "unimodal" else 2)
    assert [n for n in tr.names if "_dul_" in n][:8] == ["audio_net." + k for k in dr.DUL_NAMES]
    f32 = dtype == "f32"
    for st in range(cfg["steps"]):
        spec, image, label = _gbatch(cfg, st)
        tr.step(spec, image, label, pe_eps=_geps(cfg, st))
        r = tr.read()
        pre = f"s{st}."
        later = st > 0
        if later and not f32:
            assert np.isfinite(r["out"]).all() and np.isfinite(r["total_norm"]) and np.isfinite(r["regurize_a"])
            continue
        lt = (1e-2 if later else 5e-4) if f32 else 0.2
        ls = lt if f32 else 5e-2
        tn = float(g[pre + "total_norm"])
        print(name, dtype, st, "logits", float(np.abs(r["out"] - g[pre + "out"]).max()), "loss", r["loss_f"], float(g[pre + "loss_f"]),
              "total_norm", r["total_norm"], tn, "reg_a", r["regurize_a"], float(g[pre + "reg_a"]))
        np.testing.assert_allclose(r["out"], g[pre + "out"], rtol=lt, atol=lt)
        np.testing.assert_allclose(r["loss_f"], g[pre + "loss_f"], rtol=ls, atol=ls)
        np.testing.assert_allclose(r["regurize_a"], g[pre + "reg_a"], rtol=ls)
        if kind != "unimodal":
            np.testing.assert_allclose(r["regurize_v"], g[pre + "reg_v"], rtol=ls)
        else:
            assert "regurize_v" not in r
        if kind == "mtl":
            for k in ("out_a", "out_v"):
                np.testing.assert_allclose(r[k], g[pre + k], rtol=lt, atol=lt)
            for k in ("loss_a", "loss_v"):
                np.testing.assert_allclose(r[k], g[pre + k], rtol=ls, atol=ls)
        nt = (2e-2 if later else 3e-3) if f32 else 4e-2
        np.testing.assert_allclose(r["total_norm"], tn, rtol=nt)
        np.testing.assert_allclose(r["audio_grad_sum"], g[pre + "audio_grad_sum"], rtol=2 * nt)
        if kind != "unimodal":
            np.testing.assert_allclose(r["visual_grad_sum"], g[pre + "visual_grad_sum"], rtol=2 * nt)
        names = [str(n) for n in g[pre + "grad_names"]]
        gt = (6e-2 if later else 1e-2) if f32 else 0.3
        clip = min(1.0, 40.0 / (tn + 1e-6))
        worst, worst_n = 0.0, None
        for i, n in enumerate(names):
            want = float(g[pre + "grad_norm"][i]) * clip
            dev_ = abs(r["grad_norm"][n] - want) / (want + 1e-30)
            if "_dul_" in n and not n.endswith(".0.bias") and dev_ > worst:
                worst, worst_n = dev_, n
            assert abs(r["grad_norm"][n] - want) <= gt * want + 1e-5 * clip * tn, (n, r["grad_norm"][n], want)
            if n.endswith("_dul_backbone.0.bias"):  # the named departure: exactly zero where torch leaves rounding noise
                assert r["grad_norm"][n] == 0.0 and want < 1e-5 * clip * tn
        print(name, dtype, st, "worst norm deviation among the branch's tensors", worst, worst_n)
    last = f"s{cfg['steps'] - 1}."
    names = [str(n) for n in g[last + "grad_names"]]
    ps = g[last + "param_sums"]
    sd = model.state_dict()
    for i, n in enumerate(names):
        got = sd[n].double().abs().sum().item()
        np.testing.assert_allclose(got, ps[i][1], rtol=1e-3 if f32 else 2e-3, err_msg=n)
    for k in [k[len(last + "buf."):] for k in g.files if k.startswith(last + "buf.")]:  # the two stacks' BatchNorm buffers
        tolr, tola = (2e-3, 1e-3) if f32 else (5e-2, 3e-2)
        np.testing.assert_allclose(sd[k].cpu().numpy().astype(np.float64), g[last + "buf." + k], rtol=tolr, atol=tola, err_msg=k)
    spec, image, label = _gbatch(cfg, 1000)
    tr.valid([(spec, image, label)])
    et = 1e-2 if f32 else 0.2
    np.testing.assert_allclose(tr.out.cpu().numpy(), g["eval.out"], rtol=et, atol=et)


def _state_bytes(model, tr):
    torch.cuda.synchronize()
    return [tr.params.clone(), tr.momentum.clone()] + [b.clone().float() for b in model.buffers()]


def _run_steps(tr, cfg, steps):
    for st in steps:
        tr.step(*_gbatch(cfg, st))


@pytest.mark.parametrize("kind,fusion", [("unimodal", "concat"), ("joint", "concat")])
def test_trainer_same_seed_identical_and_resume(kind, fusion):
    """The generator's noise: two runs with the same seed give identical bytes (parameters, momentum, buffers), another seed does
    not, and a run saved after step 1 and resumed in a new trainer continues bit for bit through step 3."""
    cfg = dict(seed=0, batch=4, spec_hw=[65, 47], frames=1 if kind == "unimodal" else 3, image_hw=[64, 64], n_classes=6)
    ma, ta = _pe_trainer(kind, fusion, "bf16", 1e-2, seed=11)
    _run_steps(ta, cfg, range(3))
    A = _state_bytes(ma, ta)
    mb, tb = _pe_trainer(kind, fusion, "bf16", 1e-2, seed=11)
    _run_steps(tb, cfg, range(1))
    ck_t, ck_m = tb.state_dict(), {k: v.clone() for k, v in mb.state_dict().items()}
    assert ck_t["pe"] is True and ck_t["pe_seed"] == 11 and ck_t["steps"] == 1
    _run_steps(tb, cfg, range(1, 3))
    for a, b in zip(A, _state_bytes(mb, tb)):
        assert _same_bits(a, b)
    mc, tc = _pe_trainer(kind, fusion, "bf16", 1e-2, seed=99)  # another key: the checkpoint's replaces it
    mc.load_state_dict(ck_m)
    tc.load_state_dict(ck_t)
    assert tc.seed == 11 and tc.steps == 1
    _run_steps(tc, cfg, range(1, 3))
    for a, c in zip(A, _state_bytes(mc, tc)):
        assert _same_bits(a, c)
    md, td = _pe_trainer(kind, fusion, "bf16", 1e-2, seed=12)
    _run_steps(td, cfg, range(3))
    assert not _same_bits(A[0], _state_bytes(md, td)[0])
    # a checkpoint with the branch into a trainer without it, and the reverse: refused
    m0, t0 = _pe_trainer(kind, fusion, "bf16", 0.0, pe=0)
    with pytest.raises(L.GdlError, match="probabilistic"):
        t0.load_state_dict(ck_t)
    with pytest.raises(L.GdlError, match="probabilistic"):
        tc.load_state_dict(t0.state_dict())


def pe_off_digest(kind):
    """sha256 of (parameters, momentum, BatchNorm buffers) after two bf16 steps of the runner on a model WITHOUT the branch, built
    from the fixtures' state with calls that exist on the commit before the branch too (tools/bench_dul.py --digest runs this
    very function on a checkout of that commit; tests/golden/dul_pe_off_parent.json holds what it printed there)."""
    import hashlib

    from gdl.trainer import DGLTrainer
    from gdl.unimodal import UnimodalTrainer
    from models.basic_model import AVClassifier, AVClassifier_DGL

    args = argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="audio" if kind == "unimodal" else "full", batch_size=4)
    model = (AVClassifier if kind == "joint" else AVClassifier_DGL)(args)
    ps, bs = fx.model_state(6, "concat_dgl" if kind == "unimodal" else "concat")
    sd = {**ps, **bs}
    if kind == "unimodal":
        sd = {k: v for k, v in sd.items() if k.startswith(("fusion_module.", "audio_net."))}
        sd.update(fx.make_state({"audio_classifier.weight": (6, 512), "audio_classifier.bias": (6,)}))
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    model = model.to(DEV).train()
    for n in ("audio_net", "visual_net"):
        if getattr(model, n, None) is not None:
            getattr(model, n).gdl_dtype = "bf16"
    tr = UnimodalTrainer(model, lr=2e-3) if kind == "unimodal" else DGLTrainer(model, lr=2e-3, mode="joint")
    cfg = dict(seed=0, batch=4, spec_hw=[65, 47], frames=1 if kind == "unimodal" else 2, image_hw=[64, 64], n_classes=6)
    for st in range(2):
        tr.step(*_gbatch(cfg, st))
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in [tr.params, tr.momentum] + [b.float() for b in model.buffers()]:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest(), tr


@pytest.mark.parametrize("kind", ["unimodal", "joint"])
def test_trainer_pe_off_is_the_parent_step(kind):
    """With the switch off a UnimodalTrainer step and a joint step give the bytes the commit before the branch gave (recorded
    there on an MI355X: tests/golden/dul_pe_off_parent.json), the trainer owns no stage, keeps the 60-tensor encoders, and a
    model whose args say pe = 0 allocates exactly what a model whose args have no such attribute allocates."""
    import gc

    with open(os.path.join(GOLD, "dul_pe_off_parent.json")) as fh:
        want = json.load(fh)[kind]
    got, tr = pe_off_digest(kind)
    assert got == want
    assert not tr.pe and tr.dul is None and not any("_dul_" in n for n in tr.names)
    assert len(tr.names) == tr.nf + (60 if kind == "unimodal" else 120)
    assert "regurize_a" not in tr.read()
    cfg = dict(seed=0, batch=4, spec_hw=[65, 47], frames=1 if kind == "unimodal" else 2, image_hw=[64, 64], n_classes=6)
    with pytest.raises(L.GdlError):
        tr.step(*_gbatch(cfg, 0), pe_eps=(None, None))
    del tr
    mem = []
    for with_attr in (False, True, False):
        gc.collect()
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        model, t2 = _pe_trainer(kind, "concat", "bf16", 0.0, pe=0, with_pe_attr=with_attr)
        _run_steps(t2, cfg, range(2))
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated() - m0)
        del model, t2
    assert mem[1] == mem[2], mem  # (the first trainer of a process also pays for the shared chain streams' first use)


@pytest.mark.parametrize("form", ["dgl", "dgl_keep_head_uni", "joint_gated", "joint_film", "joint_sum"])
def test_trainer_other_forms_run_to_run(form):
    """The forms of the step the goldens do not cover, with the branch on (the stage is head-independent: the same hook): the DGL
    step itself (early backward), drop_head_uni=False, and the joint step with the sum, gated and FiLM heads -- two steps each,
    finite, the regulariser reported, the branch's tensors trained, and two runs with one seed identical to the byte."""
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier, AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    cfg = dict(seed=0, batch=4, spec_hw=[65, 47], frames=2, image_hw=[64, 64], n_classes=6)
    res = []
    for _ in range(2):
        setup_seed(0)
        fusion = form.split("_")[1] if form.startswith("joint") else "concat"
        args = argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality="full", batch_size=4, pe=1)
        model = (AVClassifier if form.startswith("joint") else AVClassifier_DGL)(args)
        model.apply(weight_init)
        model = model.to(DEV).train()
        kw = dict(mode="joint") if form.startswith("joint") else dict(mode="dgl", drop_head_uni=form == "dgl")
        tr = DGLTrainer(model, lr=2e-3, dtype="bf16", beta=1e-2, seed=3, **kw)
        w0 = model.audio_net.mu_dul_backbone[0].weight.detach().clone()
        _run_steps(tr, cfg, range(2))
        r = tr.read()
        assert np.isfinite(r["out"]).all() and np.isfinite(r["total_norm"]) and r["regurize_a"] > 0 and r["regurize_v"] > 0
        assert r["grad_norm"]["audio_net.mu_dul_backbone.0.weight"] > 0 and r["grad_norm"]["visual_net.logvar_dul_backbone.1.bias"] > 0
        assert not torch.equal(w0, model.audio_net.mu_dul_backbone[0].weight.detach())
        res.append(_state_bytes(model, tr))
    for a, b in zip(*res):
        assert _same_bits(a, b)


def test_trainer_valid_is_head_of_dul_eval_by_hand():
    from gdl.encoder import EncoderEngine

    cfg = dict(seed=0, batch=4, spec_hw=[65, 47], frames=1, image_hw=[64, 64], n_classes=6)
    model, tr = _pe_trainer("unimodal", "concat", "bf16", 1e-5)
    _run_steps(tr, cfg, range(1))  # (running statistics that are no longer the initial ones)
    spec, image, label = _gbatch(cfg, 1000)
    tr.valid([(spec, image, label)])
    got = tr.out.clone()
    net = model.audio_net
    eng = EncoderEngine("audio", "bf16", 4, 1, 65, 47, DEV)
    bns = net._bn_layers()
    eng.set_params([p.data for p in net.engine_parameters()], [b.running_mean for b in bns], [b.running_var for b in bns],
                   [b.num_batches_tracked for b in bns])
    feat, _ = eng.forward(spec.unsqueeze(1), False)
    bn = net.mu_dul_backbone[1]
    sc, sh, f2, out = (torch.empty(512, device=DEV), torch.empty(512, device=DEV), torch.empty(4, 512, device=DEV), torch.empty(4, 6, device=DEV))
    st = L.cur_stream()
    L.call("gdl_bn_finalize_eval", 512, L.ptr(bn.weight.data), L.ptr(bn.bias.data), 1e-5, L.ptr(bn.running_mean), L.ptr(bn.running_var),
           L.ptr(sc), L.ptr(sh), st)
    L.call("gdl_dul_eval", L.ptr(feat), L.ptr(net.mu_dul_backbone[0].weight.data), L.ptr(net.mu_dul_backbone[0].bias.data), L.ptr(sc),
           L.ptr(sh), L.ptr(f2), 4, 512, st)
    L.call("gdl_head_cls_fwd", L.ptr(f2), L.ptr(model.audio_classifier.weight.data), L.ptr(model.audio_classifier.bias.data), L.ptr(out),
           4, 6, 512, st)
    torch.cuda.synchronize()
    assert _same_bits(got, out)
    # ... and it is the mu stack that is evaluated, not the identity
    assert float((f2 - feat).abs().max()) > 1e-2


def test_trainer_refusals():
    """What the branch is not built for raises GdlError before any launch, never ignored."""
    from gdl.mla import MLATrainer
    from gdl.probe import extract_features
    from gdl.prototypes import Prototypes
    from gdl.trainer import DGLTrainer
    from gdl.unimodal import UnimodalTrainer

    model = _pe_model("joint", "concat", "bf16")
    for kw in (dict(modulation="OGM"), dict(modulation="OGM_GE"), dict(process_group=object()),
               dict(prototypes=Prototypes(6, torch.device(DEV)))):
        with pytest.raises(L.GdlError):
            DGLTrainer(model, lr=2e-3, mode="joint", **kw)
    with pytest.raises(L.GdlError):
        extract_features(model, "audio", [])
    with pytest.raises(L.GdlError):
        from models.basic_model import AVClassifier_MLA

        mla = AVClassifier_MLA(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=4, pe=1))
        assert mla.audio_net.pe and mla.visual_net.pe
        MLATrainer(mla.to(DEV), lr=2e-3)
    plain = _pe_model("joint", "concat", "bf16", pe=0)
    with pytest.raises(L.GdlError):
        DGLTrainer(plain, lr=2e-3, mode="joint", beta=1e-5)  # beta without the stacks
    with pytest.raises(L.GdlError):
        UnimodalTrainer(_pe_model("unimodal", "concat", "bf16", pe=0), lr=2e-3, beta=1e-5)
    with pytest.raises(L.GdlError):
        UnimodalTrainer(_pe_model("unimodal", "concat", "bf16"), lr=2e-3, process_group=object())
    # the Swin visual branch has no stacks (its mirror refuses args.pe itself): a composition whose audio encoder carries them
    from models.backbone import resnet18
    from models.basic_model import AVClassifier_DGL_Swin

    args = argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=4, pe=0)
    sc = fx.SWIN_TINY2
    with pytest.raises(NotImplementedError):
        AVClassifier_DGL_Swin(argparse.Namespace(**{**vars(args), "pe": 1}))
    swin = AVClassifier_DGL_Swin(args, swin_kwargs=dict(img_size=sc["img"], patch_size=sc["patch"], embed_dim=sc["embed"],
                                                        depths=list(sc["depths"]), num_heads=list(sc["heads"]),
                                                        window_size=sc["window"], mlp_ratio=float(sc["mlp"]), drop_path_rate=0.))
    swin.audio_net = resnet18("audio", argparse.Namespace(**{**vars(args), "pe": 1}))
    with pytest.raises(L.GdlError, match="Swin"):
        DGLTrainer(swin.to(DEV), lr=2e-3)
    # a pe_eps map of the wrong shape
    model2, tr = _pe_trainer("joint", "concat", "bf16", 1e-5)
    cfg = dict(seed=0, batch=4, spec_hw=[65, 47], frames=3, image_hw=[64, 64], n_classes=6)
    with pytest.raises(L.GdlError):
        tr.step(*_gbatch(cfg, 0), pe_eps=(torch.zeros(5, 512, device=DEV), None))
    assert tr.steps == 0

