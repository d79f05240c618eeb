"""GPU tests of the linear probe: gdl.extract_features (the device feature bank), gdl_linprobe_epoch (csrc/linprobe.hip, the
fused fit) against the float64 restatement tests/probe_ref.py, and gdl.LinearProbe against the torch trajectories of
tests/golden/probe_*_tiny.npz.

The kernel bounds (probe_ref.BOUND) are not tuned to the kernels: they are 4 x the largest deviation of the torch CPU float32
fit from the float64 restatement on the same twelve runs (six (N, B, n) cases x {max_norm 40, clipping max_norm}, 2 epochs,
lr 1e-2), measured by `tools/bench_probe.py --spread` and recorded in docs/parity_log.md "Linear probe":
    deviation() = max |got - want| / max |want| per array:   W 3.34e-7   b 2.31e-7   mW 1.69e-5   mb 1.52e-5
    loss_deviation() = |got - want| / max(1, |want|):         8.93e-8
    bounds (4 x):                                             W 1.34e-6   b 9.24e-7   mW 6.76e-5   mb 6.08e-5   loss 3.57e-7
Both are float32 fits of the same arithmetic that differ in summation order only; 4 x leaves room for another order without
hiding a wrong term (a missing weight-decay, momentum or clip term moves W by 1e-4 .. 1e-1 on these cases).  The momentum
figures are larger than the weights' because in the clipping runs the buffers are sums of terms that nearly cancel.
"""
import argparse
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import probe_ref as R
from gdl import _lib as L
from gpu_util import DEV, dev, relerr
from oracle import fixtures as fx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TINY = ((65, 47), 2, (64, 64))  # spec_hw, frames, image_hw of the tiny fixtures


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


# ------------------------------------------------------------------ extraction
@functools.lru_cache(maxsize=None)
def _model():
    from models.basic_model import AVClassifier_DGL

    P, Bf = fx.model_state(6, "concat_dgl")
    model = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=4))
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in {**P, **Bf}.items()})
    return model.to(DEV).train()  # (left in train mode: the extraction must not care)


def _batches(sizes=(4, 4, 4)):
    out = []
    for seed, B in enumerate(sizes):
        spec, image, label = fx.make_batch(seed, 4, *TINY, 6)
        out.append((dev(spec[:B]), dev(image[:B]), torch.from_numpy(label[:B]).to(DEV)))
    return out


def _engine_features(model, modality, batches, dtype):
    """EncoderEngine.forward(x, False) per batch, each on an engine of its own"""
    from gdl.encoder import EncoderEngine

    net = getattr(model, modality + "_net")
    bns = net._bn_layers()
    out = []
    for spec, image, _ in batches:
        x = spec.unsqueeze(1) if modality == "audio" else image
        T, H, W = (1, x.shape[2], x.shape[3]) if modality == "audio" else tuple(x.shape[2:])
        eng = EncoderEngine(modality, dtype, x.shape[0], T, H, W, DEV)
        eng.set_params([p.data for p in net.parameters()], [b.running_mean for b in bns], [b.running_var for b in bns],
                       [b.num_batches_tracked for b in bns])
        out.append(eng.forward(x, False)[0].cpu().numpy())
        torch.cuda.synchronize()
    return np.concatenate(out)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("modality", ["audio", "visual"])
def test_extract_features(modality, dtype):
    """The bank is bit-equal to EncoderEngine.forward(x, False) per batch at the same engine dtype; against the reference's
    eval-mode pooled features it keeps the bounds of tests/test_step_gpu.py::test_encoder_golden's eval-mode comparison
    (relerr < 2e-4 in f32, < 4e-2 in bf16); the labels arrive; the encoder -- parameters and BatchNorm buffers -- is
    bit-unchanged after extract_features + fit."""
    import gdl

    model, g = _model(), _gold(f"probe_{modality}_tiny")
    before = {k: v.clone() for k, v in model.state_dict().items()}
    batches = _batches()
    bank = gdl.extract_features(model, modality, batches, dtype=dtype)
    assert bank.N == 12 and bank.features.dtype == torch.float32 and bank.modality == modality
    got = bank.features.cpu().numpy()
    assert np.array_equal(bank.labels.cpu().numpy(), g["labels"])
    assert np.array_equal(got, _engine_features(model, modality, batches, dtype))
    r = relerr(got, g["features"])
    print(f"probe extraction {modality} {dtype}: relerr vs the reference's eval features {r:.3g}")
    assert r < (2e-4 if dtype == "f32" else 4e-2), r
    probe = gdl.LinearProbe(6, DEV, seed=1)
    losses = probe.fit(bank, 2, batch_size=4, lr=1e-2)
    assert len(losses) == 2 and np.isfinite(losses).all()
    after = model.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    assert model.training


def test_extract_features_ragged_last_batch_and_default_dtype():
    """A last batch of another size re-plans the engine; dtype=None is the encoder's own gdl_dtype; the other modality's
    tensor may be None."""
    import gdl

    model = _model()
    batches = [(s, None, y) for s, _, y in _batches((4, 3))]
    bank = gdl.extract_features(model, "audio", batches)
    assert bank.N == 7
    want = _engine_features(model, "audio", batches, model.audio_net.gdl_dtype)
    assert np.array_equal(bank.features.cpu().numpy(), want)
    with pytest.raises(L.GdlError, match="audio encoder takes"):
        gdl.extract_features(model, "audio", [(None, batches[0][0], batches[0][2])])


# ------------------------------------------------------------------ gdl_linprobe_epoch against the restatement
def _epochs(bank, labels, order, W, b, mW=None, mb=None, lr=1e-2, mu=0.9, wd=1e-4, max_norm=40.0, n=None):
    """order [epochs, steps, B] through the C ABI, an epoch per call; returns (W, b, mW, mb, epoch mean losses) as numpy."""
    lib = L.load()
    n = W.shape[0] if n is None else n
    E, steps, B = order.shape
    bank_d, lab_d, ord_d = dev(bank), torch.from_numpy(labels).to(DEV), torch.from_numpy(order).to(DEV)
    Wd, bd = dev(W), dev(b)
    mWd = torch.zeros_like(Wd) if mW is None else dev(mW)
    mbd = torch.zeros_like(bd) if mb is None else dev(mb)
    acc = torch.zeros((E, 2), dtype=torch.float64, device=DEV)
    wsb = lib.gdl_linprobe_workspace_bytes(B, n)
    assert wsb > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    for e in range(E):
        L.call("gdl_linprobe_epoch", L.ptr(bank_d), L.ptr(lab_d), bank.shape[0], ord_d[e].data_ptr(), steps, B, L.ptr(Wd), L.ptr(bd),
               L.ptr(mWd), L.ptr(mbd), n, lr, mu, wd, max_norm, acc[e].data_ptr(), L.ptr(ws), wsb, L.cur_stream())
    a = acc.cpu().numpy()
    assert (a[:, 1] == steps).all()
    return Wd.cpu().numpy(), bd.cpu().numpy(), mWd.cpu().numpy(), mbd.cpu().numpy(), a[:, 0] / a[:, 1]


@functools.lru_cache(maxsize=None)
def _reference(case, max_norm):
    bank, labels, W, b, order = R.synthetic_case(*case)
    return R.fit(bank, labels, order, W, b, max_norm=max_norm, **R.HYPER)


def _compare(tag, got, traj, bound):
    W, b, mW, mb, losses = got
    figs = {k: R.deviation(v, traj[-1][k]) for k, v in (("W", W), ("b", b), ("mW", mW), ("mb", mb))}
    figs["loss"] = max(R.loss_deviation(l, t["loss"]) for l, t in zip(losses, traj))
    print(f"linprobe {tag}: " + "  ".join(f"{k} {v:.3g} (bound {bound[k]:.3g})" for k, v in figs.items()))
    for k, v in figs.items():
        assert v < bound[k], (tag, k, v, bound[k])


@pytest.mark.parametrize("max_norm", [40.0, R.CLIP_NORM])
@pytest.mark.parametrize("case", R.CASES)
def test_linprobe_epoch_matches_restatement(case, max_norm):
    """W, b, both momentum buffers after 2 epochs and both epoch losses against probe_ref.fit, within probe_ref.BOUND (module
    docstring).  At the clipping max_norm every step of every case clips -- except (5, 1, 1), whose single class makes every
    gradient exactly zero (softmax of one logit is 1): there the run checks that a zero norm divides cleanly."""
    bank, labels, W, b, order = R.synthetic_case(*case)
    traj = _reference(case, max_norm)
    norms = np.concatenate([t["norms"] for t in traj])
    if case[2] > 1:
        assert (norms > R.CLIP_NORM).all() and (norms < 40.0).all()  # the small max_norm clips always, 40 never
    got = _epochs(bank, labels, order, W, b, max_norm=max_norm, **R.HYPER)
    _compare(f"{case} max_norm {max_norm}", got, traj, R.BOUND)


def test_linprobe_epoch_refuses_513_classes_and_touches_nothing():
    lib = L.load()
    n, B = 513, 4
    bufs = [torch.full(s, float("nan"), device=DEV) for s in ((n, 512), (n,), (n, 512), (n,))]
    acc = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.full((1 << 22,), float("nan"), device=DEV)
    bank, labels = torch.zeros((8, 512), device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    order = torch.zeros((2, B), dtype=torch.int32, device=DEV)
    rc = lib.gdl_linprobe_epoch(L.ptr(bank), L.ptr(labels), 8, L.ptr(order), 2, B, *[L.ptr(t) for t in bufs], n, 1e-2, 0.9, 1e-4, 40.0,
                                L.ptr(acc), L.ptr(ws), ws.numel() * 4, L.cur_stream())
    assert rc == 1 and b"n_classes" in lib.gdl_last_error()  # GDL_ERR_ARG
    torch.cuda.synchronize()
    for t in bufs + [acc, ws]:
        assert bool(torch.isnan(t).all())
    assert lib.gdl_linprobe_workspace_bytes(B, n) == 0


@pytest.mark.parametrize("bad", [6, -1])
def test_linprobe_epoch_label_out_of_range(bad):
    """The epoch whose steps meet the label has a NaN loss; the sample contributes its softmax without a one-hot term and the
    other samples as always: the state still matches the restatement (which restates exactly that)."""
    bank, labels, W, b, order = R.synthetic_case(12, 4, 6)
    labels = labels.copy()
    labels[order[0, 1, 2]] = bad
    traj = R.fit(bank, labels, order, W, b, max_norm=40.0, **R.HYPER)
    W1, b1, mW1, mb1, losses = _epochs(bank, labels, order, W, b, max_norm=40.0, **R.HYPER)
    assert np.isnan(losses).all() and all(np.isnan(t["loss"]) for t in traj)  # (both epochs visit the row)
    for k, v in (("W", W1), ("b", b1), ("mW", mW1), ("mb", mb1)):
        d = R.deviation(v, traj[-1][k])
        assert np.isfinite(v).all() and d < R.BOUND[k], (k, d)
    clean = _reference((12, 4, 6), 40.0)
    assert R.deviation(W1, clean[-1]["W"]) > 1e-4  # (the missing one-hot term is visible: the comparison above is not vacuous)


def test_linprobe_epoch_zero_steps_and_repeatability():
    """steps = 0 launches nothing and adds nothing; two runs from the same state and table are bit-identical."""
    bank, labels, W, b, order = R.synthetic_case(300, 64, 34)
    a = _epochs(bank, labels, order, W, b, max_norm=R.CLIP_NORM, **R.HYPER)
    c = _epochs(bank, labels, order, W, b, max_norm=R.CLIP_NORM, **R.HYPER)
    for x, y in zip(a, c):
        assert np.array_equal(x, y)
    lib = L.load()
    Wd, bd = dev(W), dev(b)
    mW, mb = torch.zeros_like(Wd), torch.zeros_like(bd)
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    ws = torch.zeros(lib.gdl_linprobe_workspace_bytes(64, 34), dtype=torch.uint8, device=DEV)
    L.call("gdl_linprobe_epoch", L.ptr(dev(bank)), L.ptr(torch.from_numpy(labels).to(DEV)), 300, None, 0, 64, L.ptr(Wd), L.ptr(bd),
           L.ptr(mW), L.ptr(mb), 34, 1e-2, 0.9, 1e-4, 40.0, L.ptr(acc), L.ptr(ws), ws.numel(), L.cur_stream())
    assert np.array_equal(Wd.cpu().numpy(), W) and np.array_equal(acc.cpu().numpy(), np.zeros(2))


# ------------------------------------------------------------------ gdl.LinearProbe
@pytest.mark.parametrize("run", ["n40", "clip"])
@pytest.mark.parametrize("name", ["probe_audio_tiny", "probe_visual_tiny"])
def test_linear_probe_golden_trajectory(name, run):
    """gdl.LinearProbe(6, seed=0) starts at the fixture's W0 / zero bias (bitwise: the weight_init rule on the seeded generator)
    and follows the fixture's torch float32 trajectory over 3 epochs, an epoch per fit() call with the state carried.
    Bounds: probe_ref.GOLDEN32_DEV is the fixtures' own float32 noise (their largest deviation from the float64 restatement,
    measured on the CPU: W 1.62e-7, b 7.22e-7, mW 3.11e-7, mb 3.74e-7, loss 7.75e-8; tests/test_probe_cpu.py pins it).  The
    probe is held to 4 x that against the restatement -- the rule of the kernel tests above -- and to 5 x that against the
    fixture, which is itself up to 1 x away from the restatement."""
    import gdl

    g = _gold(name)
    cfg = json.loads(str(g["config"]))
    vs_ref = {k: 4.0 * v for k, v in R.GOLDEN32_DEV.items()}
    vs_fixture = {k: 5.0 * v for k, v in R.GOLDEN32_DEV.items()}
    bank = gdl.FeatureBank(dev(g["features"]), torch.from_numpy(g["labels"]).to(DEV))
    probe = gdl.LinearProbe(6, DEV, seed=0)
    assert np.array_equal(probe.weight.cpu().numpy(), g["W0"]) and not probe.bias.any()
    mn = cfg["max_norm"] if run == "n40" else cfg["clip_norm"]
    traj = R.fit(g["features"], g["labels"], g["order"], g["W0"], g["b0"], lr=cfg["lr"], mu=cfg["momentum"],
                 wd=cfg["weight_decay"], max_norm=mn)
    for e in range(3):
        (loss,) = probe.fit(bank, 1, batch_size=4, lr=cfg["lr"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"],
                            max_norm=mn, order=g["order"][e:e + 1])
        sd = probe.state_dict()
        assert sd["epoch"] == e + 1
        got = (sd["weight"].cpu().numpy(), sd["bias"].cpu().numpy(), sd["momentum_weight"].cpu().numpy(),
               sd["momentum_bias"].cpu().numpy(), [loss])
        want = [{k: g[f"{run}.e{e}.{k}"] for k in ("W", "b", "mW", "mb", "loss")}]
        _compare(f"{name} {run} epoch {e} vs fixture", got, want, vs_fixture)
        _compare(f"{name} {run} epoch {e} vs float64", got, traj[e:e + 1], vs_ref)
    # the same table drawn by the probe itself (order=None) from the same seed: the same bits as the explicit table
    p2 = gdl.LinearProbe(6, DEV, seed=0)
    p2.fit(bank, 3, batch_size=4, lr=cfg["lr"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"], max_norm=mn)
    assert torch.equal(p2.weight, probe.weight) and torch.equal(p2.momentum_bias, probe.momentum_bias)


def _state_equal(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in ("weight", "bias", "momentum_weight", "momentum_bias")) and sa["epoch"] == sb["epoch"]


def test_linear_probe_is_reproducible_and_resumes_bit_equal():
    import gdl

    bank_np, labels, _, _, _ = R.synthetic_case(300, 64, 34)
    bank = gdl.FeatureBank(dev(bank_np), torch.from_numpy(labels).to(DEV))
    lrs = [gdl.multistep_lr(1e-2, [2], 0.1, e) for e in range(3)]
    assert lrs[0] != lrs[1]
    a, b = gdl.LinearProbe(34, DEV, seed=7), gdl.LinearProbe(34, DEV, seed=7)
    la, lb = a.fit(bank, 3, lr=lrs), b.fit(bank, 3, lr=lrs)
    assert la == lb and _state_equal(a, b) and np.isfinite(la).all()  # two fits from one seed
    assert not _state_equal(a, gdl.LinearProbe(34, DEV, seed=8))
    # a checkpoint after epoch 1, resumed in another probe object
    c = gdl.LinearProbe(34, DEV, seed=7)
    l1 = c.fit(bank, 1, lr=lrs[:1])
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in c.state_dict().items()}
    d = gdl.LinearProbe(34, DEV, seed=99)
    d.load_state_dict(sd)
    l2 = d.fit(bank, 2, lr=lrs[1:])
    assert l1 + l2 == la and _state_equal(d, a)
    # ... and with an explicit table (no generator involved)
    tab = gdl.probe_order(300, 64, 3, torch.Generator().manual_seed(3))
    e, f = gdl.LinearProbe(34, DEV, seed=7), gdl.LinearProbe(34, DEV, seed=7)
    e.fit(bank, 3, lr=lrs, order=tab)
    f.fit(bank, 1, lr=lrs[:1], order=tab[:1])
    h = gdl.LinearProbe(34, DEV, seed=7)
    h.load_state_dict(f.state_dict())
    h.fit(bank, 2, lr=lrs[1:], order=tab[1:])
    assert _state_equal(h, e)
    with pytest.raises(L.GdlError, match="outside"):
        e.fit(bank, 1, order=np.full((1, 1, 64), 300))
    with pytest.raises(L.GdlError, match="one value per epoch"):
        e.fit(bank, 2, lr=[1e-3])


def test_linear_probe_score():
    """Against np.argmax (first maximum) of the logits gdl_head_cls_fwd gives, in chunks with a ragged last one; an all-zero
    probe ties every logit: class 0 must win and the accuracy is the share of label 0."""
    import gdl

    bank_np, labels, W, b, _ = R.synthetic_case(300, 64, 34)
    bank = gdl.FeatureBank(dev(bank_np), torch.from_numpy(labels).to(DEV))
    probe = gdl.LinearProbe(34, DEV)
    probe.load_state_dict(dict(weight=torch.from_numpy(W), bias=torch.from_numpy(b), momentum_weight=torch.zeros(34, 512),
                               momentum_bias=torch.zeros(34), epoch=0))
    out = torch.empty((300, 34), device=DEV)
    L.call("gdl_head_cls_fwd", L.ptr(bank.features), L.ptr(probe.weight), L.ptr(probe.bias), L.ptr(out), 300, 34, 512, L.cur_stream())
    logits = out.cpu().numpy()
    np.testing.assert_allclose(logits, bank_np.astype(np.float64) @ W.astype(np.float64).T + b, rtol=0, atol=1e-4)
    pred = logits.argmax(axis=1)
    want = np.stack([np.bincount(labels, minlength=34), np.bincount(labels[pred == labels], minlength=34)])
    for chunk in (4096, 128):
        acc, counts = probe.score(bank, chunk=chunk)
        assert counts.dtype == np.int64 and np.array_equal(counts, want)
        assert acc == (pred == labels).mean()
    zero = gdl.LinearProbe(34, DEV)
    zero.weight.zero_()
    acc, counts = zero.score(bank)
    assert counts[1, 0] == (labels == 0).sum() > 0 and counts[1, 1:].sum() == 0
    assert acc == (labels == 0).mean()
