"""GPU tests of the unimodal baselines (the audio encoder alone / the visual encoder alone with a Linear(512, n) classifier,
trained by main.py's single cross-entropy): the classifier's entry points of the C ABI against float64 restatements, the fused
training-step launch against the three-call path bit for bit, UnimodalTrainer against the step goldens
(tests/golden/make_golden_unimodal.py), the drop-in autograd path against the runner, valid() and checkpoints."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as fx

pytestmark = pytest.mark.gpu

from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [(5, 6), (33, 34), (4, 309), (64, 400), (65, 6), (257, 6), (257, 34)]  # (B, n): see test_head_float64
NAN = float("nan")


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ the classifier's entry points
_HEAD = {}


def _head_case(B, n):
    """(f, W, b, g_out, labels) of one size, made once on the device and left unchanged: features randn.clamp_min(0), upstream
    gradient randn / B (as test_joint_head_float64)."""
    if (B, n) not in _HEAD:
        gen = torch.Generator(device=DEV).manual_seed(1000 * B + n)
        W = torch.randn(n, 512, generator=gen, device=DEV) * 0.05
        b = torch.randn(n, generator=gen, device=DEV) * 0.1
        f = torch.randn(B, 512, generator=gen, device=DEV).clamp_min(0)
        go = torch.randn(B, n, generator=gen, device=DEV) / B
        lab = torch.randint(0, n, (B,), generator=gen, device=DEV)
        _HEAD[(B, n)] = (f, W, b, go, lab)
    return _HEAD[(B, n)]


def _cls_fwd(f, W, b):
    out = torch.full((f.shape[0], W.shape[0]), NAN, device=DEV)
    L.call("gdl_head_cls_fwd", L.ptr(f), L.ptr(W), L.ptr(b), L.ptr(out), f.shape[0], W.shape[0], 512, L.cur_stream())
    return out


def _cls_bwd(f, W, go, want=(True, True, True)):
    """(df, dW, db) buffers pre-filled with NaN; an output not wanted is passed as NULL (its buffer must stay NaN)."""
    B, n = f.shape[0], W.shape[0]
    bufs = [torch.full((B, 512), NAN, device=DEV), torch.full((n, 512), NAN, device=DEV), torch.full((n,), NAN, device=DEV)]
    L.call("gdl_head_cls_bwd", L.ptr(f), L.ptr(W), L.ptr(go), *(L.ptr(t) if w else None for t, w in zip(bufs, want)), B, n, 512,
           L.cur_stream())
    torch.cuda.synchronize()
    return bufs


def _check64(got, ref, key):
    """test_joint_gpu's bounds: element-wise 1e-3 / 1e-3 on logits and feature gradients"""
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-3, atol=1e-3, err_msg=key)


def _check64_param(got, ref, key):
    """... and 1e-3 of the largest element (+ 1e-6) on parameter gradients"""
    scale = float(ref.abs().max())
    assert float((got.double() - ref).abs().max()) <= 1e-3 * scale + 1e-6, key


@pytest.mark.parametrize("B,n", SIZES)
def test_head_float64(B, n):
    """gdl_head_cls_fwd / _bwd against a float64 restatement at a batch that is a multiple of nothing (5, 6), one past a
    32-sample group (33, 34), class counts that are no multiple of 8 and beyond any per-wave round (4, 309) and the largest head
    the datasets have (64, 400); (65, 6), (257, 6) and (257, 34) take gdl_head_cls_ce's loss sum to its second lane stride (lane l
    adds samples l and l + 64) and past 256 blocks.  Each optional output passed as NULL once: the others keep their bits, its buffer stays NaN."""
    f, W, b, go, _ = _head_case(B, n)
    out = _cls_fwd(f, W, b)
    df, dW, db = _cls_bwd(f, W, go)
    fd, Wd, gd = f.double(), W.double(), go.double()
    _check64(out, fd @ Wd.T + b.double(), "out")
    _check64(df, gd @ Wd, "df")
    _check64_param(dW, gd.T @ fd, "dW")
    _check64_param(db, gd.sum(0), "db")
    for skip in range(3):
        got = _cls_bwd(f, W, go, tuple(i != skip for i in range(3)))
        for i, (t, full) in enumerate(zip(got, (df, dW, db))):
            if i == skip:
                assert bool(torch.isnan(t).all()), ("touched", i)
            else:
                assert torch.equal(_bits(t), _bits(full)), (skip, i)


def _cls_ce(f, W, b, lab, scale):
    B, n = f.shape[0], W.shape[0]
    out, dl, df = torch.full((B, n), NAN, device=DEV), torch.full((B, n), NAN, device=DEV), torch.full((B, 512), NAN, device=DEV)
    loss = torch.full((1,), NAN, device=DEV)
    L.call("gdl_head_cls_ce", L.ptr(f), L.ptr(W), L.ptr(b), L.ptr(lab), scale, L.ptr(out), L.ptr(loss), L.ptr(dl), L.ptr(df), B, n,
           512, L.cur_stream())
    torch.cuda.synchronize()
    return out, loss, dl, df


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("B,n", SIZES)
def test_fused_call_equals_three_calls(B, n, scale):
    """gdl_head_cls_ce: out, dlogits and df carry the bits of gdl_head_cls_fwd + gdl_softmax_ce + gdl_head_cls_bwd; its loss is
    within 2 B 2^-23 relative of gdl_softmax_ce's (B non-negative terms: the most two summation orders can differ by); a second
    call repeats the first bit for bit, loss included."""
    f, W, b, _, lab = _head_case(B, n)
    out3 = _cls_fwd(f, W, b)
    loss3, dl3 = torch.full((1,), NAN, device=DEV), torch.full((B, n), NAN, device=DEV)
    L.call("gdl_softmax_ce", L.ptr(out3), L.ptr(lab), scale, L.ptr(loss3), L.ptr(dl3), B, n, L.cur_stream())
    df3 = _cls_bwd(f, W, dl3, (True, False, False))[0]
    out, loss, dl, df = _cls_ce(f, W, b, lab, scale)
    assert torch.equal(_bits(out), _bits(out3))
    assert torch.equal(_bits(dl), _bits(dl3))
    assert torch.equal(_bits(df), _bits(df3))
    l, l3 = float(loss.item()), float(loss3.item())
    print("loss", (B, n, scale), l, l3, abs(l - l3) / l3)
    assert np.isfinite(l) and abs(l - l3) <= 2 * B * 2.0 ** -23 * l3
    again = _cls_ce(f, W, b, lab, scale)
    for a, c in zip(again, (out, loss, dl, df)):
        assert torch.equal(_bits(a), _bits(c))


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("B,n", SIZES)
def test_fused_call_df_equals_uni_dfeat(B, n, scale):
    """gdl_head_cls_ce and gdl_head_uni_dfeat (512 features, row pitch 512) run one per-sample body (csrc/head_body.h): the
    feature gradients of the two launches are the same bits."""
    f, W, b, _, lab = _head_case(B, n)
    df_uni = torch.full((B, 512), NAN, device=DEV)
    L.call("gdl_head_uni_dfeat", L.ptr(f), L.ptr(W), 512, L.ptr(b), L.ptr(lab), scale, L.ptr(df_uni), B, n, L.cur_stream())
    df = _cls_ce(f, W, b, lab, scale)[3]
    assert torch.equal(_bits(df), _bits(df_uni))


# ------------------------------------------------------------------ the step
_STATE = {}
_TINY = dict(dataset="CREMAD", n_classes=6, spec_hw=[65, 47], frames=2, image_hw=[64, 64], batch=4, seed=0, lr=2e-3)


def _state(modality):
    """the seeded state make_golden_unimodal.py loads by name: generated once, shared, never modified"""
    if modality not in _STATE:
        P, Bf = fx.model_state(6, "concat_dgl")
        keep = ("fusion_module.", modality + "_net.")
        st = {k: v for k, v in {**P, **Bf}.items() if k.startswith(keep)}
        st.update(fx.make_state({modality + "_classifier.weight": (6, 512), modality + "_classifier.bias": (6,)}))
        _STATE[modality] = {k: torch.from_numpy(np.array(v)) for k, v in st.items()}
    return _STATE[modality]


def _make_model(modality, dtype, batch=4):
    from models.basic_model import AVClassifier_DGL

    args = argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality=modality, batch_size=batch)
    model = AVClassifier_DGL(args)
    model.load_state_dict(_state(modality), strict=True)
    model = model.to(DEV)
    getattr(model, modality + "_net").gdl_dtype = dtype
    return model


def _batch(cfg, st):
    spec, image, label = fx.make_batch(cfg["seed"] + st, cfg["batch"], cfg["spec_hw"], cfg["frames"], cfg["image_hw"],
                                       cfg["n_classes"])
    return dev(spec), dev(image), torch.from_numpy(label).to(DEV)


def _fusion(model):
    return {k: v.detach().clone() for k, v in model.fusion_module.named_parameters()}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("modality", ["audio", "visual"])
def test_unimodal_step_golden(modality, dtype):
    """UnimodalTrainer against the reference's main.py step on its own unimodal model, with the constants of
    test_joint_step_golden (tests/test_joint_gpu.py), tensor for tensor.  The fixture's total norm is the float64 norm of the
    reference's float32 gradients and its per-tensor norms are unclipped; the runner reports clipped ones.  The reference's own
    float32 / float64 spread on these fixtures is in docs/parity_log.md."""
    from gdl.unimodal import UnimodalTrainer

    g = _gold(f"uni_{modality}_tiny_b4")
    cfg = json.loads(str(g["config"]))
    model = _make_model(modality, dtype)
    model.train()
    tr = UnimodalTrainer(model, lr=cfg["lr"])
    assert tr.names[:2] == [modality + "_classifier.weight", modality + "_classifier.bias"] and len(tr.names) == 62
    f32 = dtype == "f32"
    absent = "visual_grad_sum" if modality == "audio" else "audio_grad_sum"
    present = modality + "_grad_sum"
    for st in range(cfg["steps"]):
        spec, image, label = _batch(cfg, st)
        if modality == "audio":
            tr.step(spec, None, label)  # the other modality's tensor may be None
        else:
            tr.step(None, image, label)
        r = tr.read()
        pre = f"s{st}."
        later = st > 0
        assert "out_a" not in r and "out_v" not in r
        assert r["loss_a"] == r["loss_f"] and r["loss_v"] == r["loss_f"] and r[absent] == 0.0
        if later and not f32:
            assert np.isfinite(r["out"]).all() and np.isfinite(r["total_norm"])
            continue
        lt = (1e-2 if later else 5e-4) if f32 else 0.2
        ls = lt if f32 else 5e-2
        print(modality, dtype, st, "logits", float(np.abs(r["out"] - g[pre + "out"]).max()), "loss", r["loss_f"],
              float(g[pre + "loss_f"]), "total_norm", r["total_norm"], float(g[pre + "total_norm"]), present, r[present],
              float(g[pre + present]))
        np.testing.assert_allclose(r["out"], g[pre + "out"], rtol=lt, atol=lt)
        np.testing.assert_allclose(r["loss_f"], g[pre + "loss_f"], rtol=ls, atol=ls)
        nt = (2e-2 if later else 3e-3) if f32 else 4e-2
        tn = float(g[pre + "total_norm"])
        np.testing.assert_allclose(r["total_norm"], tn, rtol=nt)
        np.testing.assert_allclose(r[present], g[pre + present], rtol=2 * nt)
        assert float(g[pre + absent]) == 0.0
        names = [str(n) for n in g[pre + "grad_names"]]
        gt = (6e-2 if later else 1e-2) if f32 else 0.3
        clip = min(1.0, 40.0 / (tn + 1e-6))
        worst = 0.0
        for i, n in enumerate(names):
            if g[pre + "grad_is_none"][i]:
                assert n.startswith("fusion_module.") and n not in r["grad_norm"]
                continue
            want = float(g[pre + "grad_norm"][i]) * clip
            worst = max(worst, abs(r["grad_norm"][n] - want) / (want + 1e-30))
            assert abs(r["grad_norm"][n] - want) <= gt * want + 1e-5 * clip * tn, (n, r["grad_norm"][n], want)
        print(modality, dtype, st, "worst per-tensor norm deviation", worst)
    last = f"s{cfg['steps'] - 1}."
    names = [str(n) for n in g[last + "grad_names"]]
    ps = g[last + "param_sums"]
    sd = model.state_dict()
    for i, n in enumerate(names):
        got = sd[n].double().abs().sum().item()
        np.testing.assert_allclose(got, ps[i][1], rtol=(2e-5 if cfg["steps"] == 1 else 1e-3) if f32 else 2e-3, err_msg=n)
    for k in [k[len(last + "buf."):] for k in g.files if k.startswith(last + "buf.")]:
        tolr, tola = (2e-3, 1e-4) if f32 else (5e-2, 3e-2)
        if cfg["steps"] > 1:
            tola = max(tola, 1e-3)
        np.testing.assert_allclose(sd[k].cpu().numpy().astype(np.float64), g[last + "buf." + k], rtol=tolr, atol=tola, err_msg=k)
    model.eval()
    spec, image, label = _batch(cfg, 1000)
    with torch.no_grad():
        ev = model(spec.unsqueeze(1), image)[0]
    et = (1e-2 if cfg["steps"] > 1 else 2e-3) if f32 else 0.2
    print(modality, dtype, "eval.out", float(np.abs(ev.cpu().numpy() - g["eval.out"]).max()))
    np.testing.assert_allclose(ev.cpu().numpy(), g["eval.out"], rtol=et, atol=et)


@pytest.mark.parametrize("modality", ["audio", "visual"])
def test_unused_fusion_tensors_stay(modality):
    """The fusion_module the reference constructs in these modes is outside the arena and bit-unchanged by the steps (no
    gradient, no weight decay), like fc_auxi in the DGL step."""
    from gdl.unimodal import UnimodalTrainer

    model = _make_model(modality, "f32")
    model.train()
    P0 = _fusion(model)
    assert len(P0) == 4
    tr = UnimodalTrainer(model, lr=_TINY["lr"])
    for st in range(2):
        tr.step(*_batch(_TINY, st))
    torch.cuda.synchronize()
    assert not [n for n in tr.names if "fusion" in n]
    for k, v in model.fusion_module.named_parameters():
        assert torch.equal(_bits(v.detach()), _bits(P0[k])), k
    with pytest.raises(ValueError):
        tr.grad("fusion_module.fc_out.weight")
    assert tr.grad(modality + "_classifier.bias").shape == (6,)
    tr.close()
    tr.close()  # idempotent


@pytest.mark.parametrize("kind", ["sgd", "Adam", "AdaGrad"])
@pytest.mark.parametrize("modality", ["audio", "visual"])
def test_dropin_step_equals_runner(modality, kind):
    """The script-style body on the mirror -- model(...)[0], one CrossEntropyLoss, backward, clip_grad_norm_, torch.optim --
    against UnimodalTrainer on the same state and batch.  Logits, loss, norms and the mean-|g| sum do not depend on the
    optimizer: the bounds of test_dropin_joint_step_equals_runner (5e-4, 3e-3, 6e-3) for all three.  The update: SGD to that
    test's 2e-5 on the parameter sums.  The first Adam / AdaGrad step moves every element by lr * g / (|g| + eps), the sign of a
    gradient whose last bits differ between the two paths (torch's cross-entropy and float32 clip against the library's), so
    element-wise agreement of two gradient computations is not defined at g ~ 0; the update is held the way
    test_runner_against_torch_optim holds it, to its bounds: torch.optim (float64, foreach=False, the script's arguments) fed
    with the runner's pre-step parameters and its clipped gradients must land where the runner did, parameters and state."""
    import torch.nn as nn
    from test_optimizers_gpu import STATE, _close  # its bounds: RTOL 1e-5, ATOL_REL 1e-6 of the tensor's largest |value|

    from gdl.unimodal import UnimodalTrainer

    cfg = _TINY
    spec, image, label = _batch(cfg, 0)
    model = _make_model(modality, "f32")
    if kind == "sgd":
        optimizer = torch.optim.SGD(model.parameters(), lr=cfg["lr"], momentum=0.9, weight_decay=1e-4)
    elif kind == "Adam":
        optimizer = torch.optim.AdamW(model.parameters(), lr=cfg["lr"], betas=(0.9, 0.999))
    else:
        optimizer = torch.optim.Adagrad(model.parameters(), lr=cfg["lr"])
    criterion = nn.CrossEntropyLoss()
    model.train()
    optimizer.zero_grad()
    out = model(spec.unsqueeze(1).float(), image.float())[0]
    loss = criterion(out, label)
    loss.backward()
    for n, p in model.named_parameters():
        assert (p.grad is None) == n.startswith("fusion_module."), n
    norms = {n: p.grad.double().norm().item() for n, p in model.named_parameters() if p.grad is not None}  # before the clip
    total = nn.utils.clip_grad_norm_(model.parameters(), max_norm=40, norm_type=2).item()
    enc_sum = sum(torch.abs(p.grad).mean().item() for p in getattr(model, modality + "_net").parameters())
    optimizer.step()
    want_out, want_loss = out.detach().cpu().numpy(), loss.item()
    want_sums = {k: v.double().abs().sum().item() for k, v in model.state_dict().items()}
    del model, optimizer, out, loss
    m2 = _make_model(modality, "f32")
    m2.train()
    tr = UnimodalTrainer(m2, lr=cfg["lr"], optimizer=kind)
    pre = tr.params.double()
    tr.step(spec, image, label)
    r = tr.read()
    np.testing.assert_allclose(r["out"], want_out, rtol=5e-4, atol=5e-4)
    np.testing.assert_allclose(r["loss_f"], want_loss, rtol=5e-4)
    np.testing.assert_allclose(r["total_norm"], total, rtol=3e-3)
    np.testing.assert_allclose(r[modality + "_grad_sum"], enc_sum, rtol=6e-3)
    assert r["visual_grad_sum" if modality == "audio" else "audio_grad_sum"] == 0.0
    clip = min(1.0, 40.0 / (total + 1e-6))
    assert set(norms) == set(tr.names)
    for n, v in norms.items():
        assert abs(r["grad_norm"][n] - v * clip) <= 3e-3 * v * clip + 1e-5 * clip * total, (n, r["grad_norm"][n], v * clip)
    if kind == "sgd":
        for k, v in m2.state_dict().items():
            np.testing.assert_allclose(v.double().abs().sum().item(), want_sums[k], rtol=2e-5, atol=1e-6, err_msg=k)
        return
    offs = tr.offsets
    shadow = [pre[offs[i]:offs[i + 1]].clone().requires_grad_() for i in range(len(tr.names))]
    opt = (torch.optim.AdamW(shadow, lr=cfg["lr"], betas=(0.9, 0.999), foreach=False) if kind == "Adam"
           else torch.optim.Adagrad(shadow, lr=cfg["lr"], foreach=False))
    for i, x in enumerate(shadow):
        x.grad = tr.grad(tr.names[i]).reshape(-1).double()
    opt.step()
    for i, (nm, x) in enumerate(zip(tr.names, shadow)):
        _close(tr.params[offs[i]:offs[i + 1]], x.detach(), nm)
        for attr, key in STATE[kind].items():
            _close(getattr(tr, attr)[offs[i]:offs[i + 1]], opt.state[x][key], f"{attr} {nm}")
    # the tensors the step does not train are where the script's optimizer left them: untouched
    for k, v in m2.fusion_module.named_parameters():
        np.testing.assert_allclose(v.double().abs().sum().item(), want_sums["fusion_module." + k], rtol=0, atol=0, err_msg=k)


@pytest.mark.parametrize("modality", ["audio", "visual"])
def test_valid(modality):
    """valid() on two tiny batches equals arg-max counting of the eval-mode logits on the host; the three accuracies are one."""
    from gdl.unimodal import UnimodalTrainer

    cfg = _TINY
    model = _make_model(modality, "f32")
    tr = UnimodalTrainer(model, lr=cfg["lr"])
    batches = [_batch(cfg, 1000), _batch(cfg, 1001)]
    acc = tr.valid(batches)
    model.eval()
    hit = tot = 0
    num = np.zeros(cfg["n_classes"])
    with torch.no_grad():
        for spec, image, label in batches:
            o = model(spec.unsqueeze(1), image)[0].cpu().numpy()
            lab = label.cpu().numpy()
            hit += int((np.argmax(o, axis=1) == lab).sum())
            tot += len(lab)
            num += np.bincount(lab, minlength=cfg["n_classes"])
    assert abs(acc[0] - hit / tot) < 1e-12 and acc[1] == acc[0] and acc[2] == acc[0]
    np.testing.assert_array_equal(tr.valid_counts[0], num)
    assert tr.valid_counts[1].sum() == hit


def test_checkpoint_visual():
    """state_dict() / load_state_dict() of a visual-only SGD trainer: a run resumed from the checkpoint continues
    bit-identically for two more steps."""
    from gdl.unimodal import UnimodalTrainer

    cfg = _TINY

    def fresh():
        m = _make_model("visual", "f32")
        m.train()
        return m, UnimodalTrainer(m, lr=cfg["lr"])

    m0, t0 = fresh()
    b = [_batch(cfg, st) for st in range(3)]
    t0.step(*b[0])
    ck_model = {k: v.clone() for k, v in m0.state_dict().items()}
    ck_opt = t0.state_dict()
    assert ck_opt["steps"] == 1 and ck_opt["optimizer"] == "sgd"
    assert ck_opt["names"][:2] == ["visual_classifier.weight", "visual_classifier.bias"]
    m1, _ = fresh()
    m1.load_state_dict(ck_model)
    t1 = UnimodalTrainer(m1, lr=cfg["lr"])  # (re-alias the arena to the loaded weights)
    t1.load_state_dict(ck_opt)
    assert t1.steps == 1
    for st in (1, 2):
        t0.step(*b[st])
        want = t0.read()
        t1.step(*b[st])
        got = t1.read()
        np.testing.assert_array_equal(got["out"], want["out"])
        assert got["total_norm"] == want["total_norm"] and got["loss_f"] == want["loss_f"]
    for k, v in m0.state_dict().items():
        assert torch.equal(v, m1.state_dict()[k]), k
    with pytest.raises(L.GdlError):
        UnimodalTrainer(_make_model("audio", "f32"), lr=cfg["lr"]).load_state_dict(ck_opt)  # another layout


def test_visual_mode_groups_frames_by_args_batch_size():
    """basic_model.py:94-95: the visual mode views the B*T frame maps as [args.batch_size, -1, C, H, W].  A [4,3,2,H,W] input on a
    model built with batch_size = 2 gives two rows, bit-equal to the same frames handed over as [2,3,4,H,W]; a frame count that
    does not divide is refused."""
    _, image, _ = _batch(_TINY, 1000)
    m2 = _make_model("visual", "f32", batch=2).eval()
    frames = image.permute(0, 2, 1, 3, 4).reshape(2, 4, 3, 64, 64).permute(0, 2, 1, 3, 4).contiguous()
    with torch.no_grad():
        got = m2(None, image)
        want = m2(None, frames)
    assert got[0].shape == (2, 6) and got[1] is got[0] and got[2] is got[0]
    assert torch.equal(_bits(got[0]), _bits(want[0]))
    with pytest.raises(RuntimeError, match="batch_size"):
        _make_model("visual", "f32", batch=3)(None, image)
