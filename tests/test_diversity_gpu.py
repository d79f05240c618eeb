"""GPU tests of the feature-diversity monitor (csrc/diversity.hip): the kernel through the C ABI against the float64 statement
of tests/diversity_ref.py on the stored values, its determinism, the epoch accumulator and the ticket counter, NaN for a
position of equal channels; the engine's and the package's entry points on a real encoder map; DGLTrainer / UnimodalTrainer
with the switch on against the reference step fixture, and bit-identical to the switch off in everything else.

Bound of every float32-against-float64 comparison of the kernel: rtol 1e-4 (as test_head_mtl_ce).  The reference
function's own float32 run is within 2.2e-6 of float64 on these inputs (tests/test_diversity_cpu.py); arithmetic on
bf16-rounded centred values would land near 1e-3 and fail.

Worst deviations measured on MI355X (kernel against diversity_ref, per image and mean, all listed shapes and kinds): f32 NHWC
2.2e-7, bf16 NHWC 2.5e-7, f32 NCHW 2.2e-7; the engine's call 9.0e-8 ... 1.6e-7; the trainer's step 0 against the reference step
fixture 7.9e-9 / 1.7e-8 (f32, audio / visual) and 4.2e-6 / 3.4e-6 (bf16, printed only).  docs/parity_log.md, "Feature-diversity
monitor", has the tables."""
import argparse
import os

import numpy as np
import pytest
import torch

import diversity_ref as dr
from gdl import _lib as L
from gpu_util import DEV, bf16_round, dev
from oracle import fixtures as fx

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diversity_ref.npz"), allow_pickle=False)
SEED = 7
RTOL = 1e-4
COMBOS = {"f32-nhwc": (L.GDL_F32, L.GDL_LAYOUT_NHWC), "bf16-nhwc": (L.GDL_BF16, L.GDL_LAYOUT_NHWC),
          "f32-nchw": (L.GDL_F32, L.GDL_LAYOUT_NCHW)}
OP_CASES = [(k, s) for k in ("relu", "shift32") for s in dr.SHAPES] + [("same", dr.SAME_SHAPE)]
# image counts that reach the mean fold's second lane stride (65) and its second lap (257), at the smallest P whose d varies
OP_CASES += [("relu", (65, 2, 1)), ("relu", (257, 2, 1))]
WORST = {}
_REF = {}


def _case(kind, shape, dt):
    """(stored values as float32 NCHW numpy, float64 reference per image, mean): computed once per (kind, shape, dtype), shared"""
    key = (kind, shape, dt)
    if key not in _REF:
        x = dr.make_map(SEED, *shape, kind)
        x = bf16_round(x) if dt == L.GDL_BF16 else x
        _REF[key] = (x,) + dr.diversity_ref(x)
    return _REF[key]


def _device_map(x, dt, layout):
    t = torch.from_numpy(x).to(DEV)
    if layout == L.GDL_LAYOUT_NCHW:
        return t.contiguous()
    return t.permute(0, 2, 3, 1).contiguous().to(L.torch_dtype(dt))


def _ws(n_img):
    return torch.zeros(L.load().gdl_feature_diversity_workspace_bytes(n_img), dtype=torch.uint8, device=DEV)


def _launch(t, dt, layout, n, P, ws, accum=None):
    per = torch.full((n,), -1.0, device=DEV)
    mean = torch.full((1,), -1.0, device=DEV)
    L.call("gdl_feature_diversity", L.ptr(t), dt, layout, n, P, 512, L.ptr(per), L.ptr(mean), L.ptr(accum), L.ptr(ws), ws.numel(),
           L.cur_stream())
    return per.cpu().numpy(), mean.cpu().numpy()[0]


def _counter(ws):
    return int(ws[:4].cpu().numpy().view(np.uint32)[0])


def _note(combo, dev_):
    WORST[combo] = max(WORST.get(combo, 0.0), dev_)
    print(f"diversity deviation [{combo}]: this case {dev_:.2e}, worst so far {WORST[combo]:.2e}")


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("kind,shape", OP_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_kernel_against_float64(kind, shape, combo):
    """per_image and the mean against diversity_ref on the very values the kernel reads (bf16: the rounded map, widened); the
    mean is the documented fold of the per-image values, bit for bit; three launches on one workspace give identical bits,
    leave the counter word zero and the accumulator at (fold of the three means, 3)."""
    dt, layout = COMBOS[combo]
    n, h, w = shape
    x, d64, m64 = _case(kind, shape, dt)
    t = _device_map(x, dt, layout)
    ws, accum = _ws(n), torch.zeros(2, device=DEV)
    runs = [_launch(t, dt, layout, n, h * w, ws, accum) for _ in range(3)]
    per, mean = runs[0]
    dev_ = max(float(np.max(np.abs(per - d64) / d64)), abs(float(mean) - m64) / m64)
    _note(combo, dev_)
    np.testing.assert_allclose(per, d64, rtol=RTOL, atol=0)
    np.testing.assert_allclose(mean, m64, rtol=RTOL, atol=0)
    assert mean.tobytes() == dr.fold_mean(per).tobytes(), (mean, dr.fold_mean(per))
    for p2, m2 in runs[1:]:
        assert p2.tobytes() == per.tobytes() and m2.tobytes() == mean.tobytes()
    assert _counter(ws) == 0
    want = np.float32(0)
    for _ in range(3):
        want = np.float32(want + mean)
    acc = accum.cpu().numpy()
    assert acc[0].tobytes() == want.tobytes() and acc[1] == 3.0, (acc, want)


def test_closed_forms_on_the_device():
    """P = 1 gives C - 1 = 511; every position equal gives 511 / P"""
    for combo, (dt, layout) in COMBOS.items():
        x, _, _ = _case("relu", (1, 1, 1), dt)
        per, mean = _launch(_device_map(x, dt, layout), dt, layout, 1, 1, _ws(1))
        np.testing.assert_allclose([per[0], mean], 511.0, rtol=RTOL)
        x, _, _ = _case("same", dr.SAME_SHAPE, dt)
        per, mean = _launch(_device_map(x, dt, layout), dt, layout, 2, 49, _ws(2))
        np.testing.assert_allclose(per, 511.0 / 49, rtol=RTOL)


@pytest.mark.parametrize("combo", list(COMBOS))
def test_zero_row_is_nan_for_that_image_alone(combo):
    """A position whose 512 channels are all equal (here: zero): NaN for its image, finite and right for the others, NaN mean
    -- never Inf -- and the next launch on the same workspace is correct."""
    dt, layout = COMBOS[combo]
    shape = (3, 7, 7)
    x, d64, m64 = _case("zero_row", shape, dt)
    i, _ = dr.zero_row_index(*shape)
    ws = _ws(3)
    per, mean = _launch(_device_map(x, dt, layout), dt, layout, 3, 49, ws)
    assert np.isnan(per[i]) and np.isnan(mean) and np.isnan(d64[i])
    ok = np.arange(3) != i
    np.testing.assert_allclose(per[ok], d64[ok], rtol=RTOL, atol=0)
    assert _counter(ws) == 0
    x2, d2, m2 = _case("relu", shape, dt)
    per, mean = _launch(_device_map(x2, dt, layout), dt, layout, 3, 49, ws)
    np.testing.assert_allclose(per, d2, rtol=RTOL, atol=0)
    np.testing.assert_allclose(mean, m2, rtol=RTOL, atol=0)
    # all channels of a position equal but not zero: the same NaN (the row is centred to exact zeros)
    x3 = x2.copy()
    x3.reshape(3, 512, 49)[0, :, 5] = x3.reshape(3, 512, 49)[0, 7, 5] + 0.7
    x3 = bf16_round(x3) if dt == L.GDL_BF16 else x3
    per, mean = _launch(_device_map(x3, dt, layout), dt, layout, 3, 49, ws)
    assert np.isnan(per[0]) and np.isfinite(per[1:]).all() and np.isnan(mean)


# ------------------------------------------------------------------ the engine and the package entry point
_STATE = {}
_TINY = dict(dataset="CREMAD", n_classes=6, spec_hw=[65, 47], frames=2, image_hw=[64, 64], batch=4, seed=0, lr=2e-3, alpha=4.0)


def _state(fusion):
    if fusion not in _STATE:
        P, Bf = fx.model_state(6, fusion + "_dgl")
        _STATE[fusion] = {k: torch.from_numpy(np.array(v)) for k, v in {**P, **Bf}.items()}
    return _STATE[fusion]


def _make_model(fusion, dtype, joint=False):
    from models.basic_model import AVClassifier, AVClassifier_DGL

    args = argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality="full", batch_size=4)
    model = (AVClassifier if joint else AVClassifier_DGL)(args)
    model.load_state_dict(_state(fusion), strict=True)
    model = model.to(DEV)
    model.audio_net.gdl_dtype = dtype
    model.visual_net.gdl_dtype = dtype
    return model.train()


def _batch(st):
    c = _TINY
    spec, image, label = fx.make_batch(c["seed"] + st, c["batch"], c["spec_hw"], c["frames"], c["image_hw"], c["n_classes"])
    return dev(spec), dev(image), torch.from_numpy(label).to(DEV)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_engine_and_function_on_an_encoder_map(dtype):
    """EncoderEngine.forward(want_fmap=True) then feature_diversity(): the engine's own buffer (NHWC, storage dtype) against
    diversity_ref on the float32 NCHW map the same forward handed out -- the same stored values, so the kernel's 1e-4 holds in
    bf16 too.  gdl.feature_diversity on that tensor (NCHW float32) and on a channels-last bf16 copy of it."""
    import gdl

    model = _make_model("concat", dtype)
    spec, image, _ = _batch(0)
    for net, x in ((model.audio_net, spec.unsqueeze(1)), (model.visual_net, image)):
        eng = net._engine(x)
        net._bind(eng)
        _, fmap = eng.forward(x, True, want_feat=False, want_fmap=True)
        mean, per = eng.feature_diversity(per_image=True)
        assert mean.dim() == 0 and mean.device.type == "cuda" and per.shape == (fmap.shape[0],)
        d64, m64 = dr.diversity_ref(fmap.cpu().numpy())
        dev_ = max(float(np.max(np.abs(per.cpu().numpy() - d64) / d64)), abs(float(mean) - m64) / m64)
        _note(f"engine-{dtype}-{net.modality}", dev_)
        np.testing.assert_allclose(per.cpu().numpy(), d64, rtol=RTOL, atol=0)
        np.testing.assert_allclose(float(mean), m64, rtol=RTOL, atol=0)
        m2 = gdl.feature_diversity(fmap)
        assert m2.dim() == 0 and m2.device.type == "cuda"
        np.testing.assert_allclose(float(m2), m64, rtol=RTOL, atol=0)
        cl = fmap.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        m3, p3 = gdl.feature_diversity(cl, per_image=True)
        np.testing.assert_allclose(p3.cpu().numpy(), dr.diversity_ref(cl.float().cpu().numpy())[0], rtol=RTOL, atol=0)
        with pytest.raises(L.GdlError, match="contiguous"):
            gdl.feature_diversity(fmap.double())
    with pytest.raises(L.GdlError, match="no CPU path"):
        gdl.feature_diversity(torch.zeros(1, 512, 2, 2))


# ------------------------------------------------------------------ the trainers
def _dgl(fusion, dtype="f32", joint=False, **kw):
    from gdl.trainer import DGLTrainer

    model = _make_model(fusion, dtype, joint)
    return DGLTrainer(model, lr=_TINY["lr"], alpha=_TINY["alpha"], mode="joint" if joint else "dgl", **kw)


def _uni(modality, dtype="f32", **kw):
    from gdl.unimodal import UnimodalTrainer
    from models.basic_model import AVClassifier_DGL

    model = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality=modality, batch_size=4))
    st = {k: v for k, v in _state("concat").items() if k.startswith(("fusion_module.", modality + "_net."))}
    st.update({k: torch.from_numpy(v) for k, v in fx.make_state({modality + "_classifier.weight": (6, 512),
                                                                  modality + "_classifier.bias": (6,)}).items()})
    model.load_state_dict(st, strict=True)
    model = model.to(DEV).train()
    getattr(model, modality + "_net").gdl_dtype = dtype
    return UnimodalTrainer(model, lr=_TINY["lr"], **kw)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainer_step_against_the_reference(dtype):
    """DGLTrainer(diversity=True), step 0 of the tiny fixture: a_diversity / v_diversity against the reference function on the
    imported reference encoders' outputs (tests/golden/make_golden_diversity.py).  f32: rtol 1e-3, SURVEY's float32 bound for
    quantities downstream of forty layers.  bf16: printed for the parity log, not asserted -- BatchNorm over 4-8 samples in
    bf16 has no bound derived here."""
    tr = _dgl("concat", dtype, diversity=True)
    tr.step(*_batch(0))
    r = tr.read()
    for k, key in (("a", "a_diversity"), ("v", "v_diversity")):
        want = float(GOLD[f"step.{k}.m64"])
        print(f"trainer {dtype} {key}: {r[key]!r} reference {want!r} deviation {abs(r[key] - want) / want:.2e}")
        assert np.isfinite(r[key])
        if dtype == "f32":
            np.testing.assert_allclose(r[key], want, rtol=1e-3, atol=0)


def _snapshot(tr, r):
    keys = [k for k in ("loss_f", "loss_a", "loss_v", "total_norm", "clip_coef", "audio_grad_sum", "visual_grad_sum") if k in r]
    return {"params": tr.params.cpu().numpy(), "grads": tr.grads.cpu().numpy(), "out": r["out"],
            "out_a": r.get("out_a", r["out"]), "out_v": r.get("out_v", r["out"]),
            "scalars": np.array([r[k] for k in keys], dtype=np.float64)}


# the form of DGLTrainer.step each case takes, as the step's phase marks show it: the early form (each encoder's backward
# behind its own forward) has no forward -> head junction and so no "fwd_done" mark; the others have it
_FORMS = {"dgl-concat-early": False, "dgl-concat-late": True, "dgl-concat-junction": True, "joint-gated": True}


@pytest.mark.parametrize("which", list(_FORMS) + ["unimodal-audio"])
def test_switch_changes_nothing_else(which):
    """Two steps with diversity=True leave the losses, the logits, the gradient sums, the gradient arena and every parameter
    bit-identical to diversity=False; off, read() has no diversity key and nothing is allocated; on, epoch_diversity() is the
    mean of the per-step read() values and resets.  Every form of the step that launches the monitor: DGL concat early (the
    default there), late (early_backward=False), with the fused loss reaching the encoders (detach_fused=False: the one-launch
    junction), the joint gated step, and the unimodal audio runner."""
    make = {"dgl-concat-early": lambda **kw: _dgl("concat", **kw),
            "dgl-concat-late": lambda **kw: _dgl("concat", early_backward=False, **kw),
            "dgl-concat-junction": lambda **kw: _dgl("concat", detach_fused=False, **kw),
            "joint-gated": lambda **kw: _dgl("gated", joint=True, **kw),
            "unimodal-audio": lambda **kw: _uni("audio", **kw)}[which]
    keys = ("a_diversity",) if which == "unimodal-audio" else ("a_diversity", "v_diversity")
    snaps, steps = {}, {k: [] for k in keys}
    for on in (False, True):
        tr = make(diversity=on)
        for st in range(2):
            tr.step(*_batch(st))
            r = tr.read()
            if on:
                assert set(k for k in r if k.endswith("_diversity")) == set(keys)
                for k in keys:
                    steps[k].append(np.float32(r[k]))
            else:
                assert not any(k.endswith("_diversity") for k in r)
        snaps[on] = _snapshot(tr, r)
        if on:
            ep = tr.epoch_diversity()
            assert set(ep) == set(keys)
            for k in keys:
                want = np.float32(np.float32(steps[k][0] + steps[k][1])) / np.float64(2)
                assert ep[k] == float(want), (k, ep[k], steps[k])
            assert all(np.isnan(v) for v in tr.epoch_diversity().values())  # reset: no step since
            if which in _FORMS:
                tr.phase_events = []
            tr.step(*_batch(2))
            again = tr.epoch_diversity(reset=False)
            assert all(again[k] == tr.read()[k] for k in keys) and tr.epoch_diversity() == again
            if which in _FORMS:  # the case ran the form of the step it is named after
                assert ("fwd_done" in [name for name, _ in tr.phase_events]) == _FORMS[which], tr.phase_events
        else:
            assert not hasattr(tr, "div") and not hasattr(tr, "div_acc")
            with pytest.raises(L.GdlError, match="off"):
                tr.epoch_diversity()
    for k in snaps[False]:
        assert snaps[False][k].tobytes() == snaps[True][k].tobytes(), k


def test_swin_branch_is_refused():
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier_DGL_Swin

    sc = fx.SWIN_TINY2
    swin = AVClassifier_DGL_Swin(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", pe=0),
                                 swin_kwargs=dict(img_size=sc["img"], patch_size=sc["patch"], embed_dim=sc["embed"],
                                                  depths=list(sc["depths"]), num_heads=list(sc["heads"]), window_size=sc["window"],
                                                  mlp_ratio=float(sc["mlp"]), drop_path_rate=0.)).to(DEV)
    with pytest.raises(L.GdlError, match="pooled tokens"):
        DGLTrainer(swin, lr=1e-3, diversity=True)
    DGLTrainer(swin, lr=1e-3).close()  # off: built as before
