"""GPU tests of the DGL ablation switches and the multi-task baseline: gdl_head_mtl_ce (the one-launch junction of the step whose
fused loss reaches the encoders) bit for bit against the three launches it replaces and against the float64 restatement
(tests/ablation_ref.py); DGLTrainer(detach_fused=..., drop_head_uni=...) against the step goldens
(tests/golden/make_golden_ablation.py); the fused junction against the three-launch junction at step level; the defaults against
a trainer built without the keywords; checkpoints; refusals."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import fixtures as fx

pytestmark = pytest.mark.gpu

import ablation_ref as ar  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
ALPHA = 2.5
OUTPUTS = ("out", "out_a", "out_v", "g_f", "g_a", "g_v", "dfa", "dfv")


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


# ------------------------------------------------------------------ gdl_head_mtl_ce
def _head_inputs(kind, B, n, seed=0):
    """Inputs of the head at the scale it sees in the step: pooled post-ReLU features (non-negative), nn.Linear's default
    initialisation scale for a 512 / 1024-wide layer (std 0.02), random labels."""
    rs = np.random.default_rng([seed, B, n, kind == "sum"])
    x = np.maximum(rs.standard_normal((B, 512), dtype=np.float32), 0)
    y = np.maximum(rs.standard_normal((B, 512), dtype=np.float32), 0)
    if kind == "concat":
        P = [(rs.standard_normal((n, 1024), dtype=np.float32) * 0.02).astype(np.float32),
             (rs.standard_normal(n, dtype=np.float32) * 0.1).astype(np.float32)]
    else:
        P = [(rs.standard_normal((n, 512), dtype=np.float32) * 0.02).astype(np.float32),
             (rs.standard_normal(n, dtype=np.float32) * 0.1).astype(np.float32),
             (rs.standard_normal((n, 512), dtype=np.float32) * 0.02).astype(np.float32),
             (rs.standard_normal(n, dtype=np.float32) * 0.1).astype(np.float32)]
    return x, y, P, rs.integers(0, n, B)


def _bufs(B, n):
    nan = float("nan")
    d = {k: torch.full((B, n), nan, device=DEV) for k in OUTPUTS[:6]}
    d.update(dfa=torch.full((B, 512), nan, device=DEV), dfv=torch.full((B, 512), nan, device=DEV),
             losses=torch.full((3,), nan, device=DEV))
    return d


def _mtl_args(kind, Pd):
    if kind == "concat":
        return L.ptr(Pd[0]), Pd[0].data_ptr() + 512 * 4, 1024, L.ptr(Pd[1]), L.ptr(Pd[1]), 0
    return L.ptr(Pd[0]), L.ptr(Pd[2]), 512, L.ptr(Pd[1]), L.ptr(Pd[3]), 1


def _fused(kind, xd, yd, Pd, ld, reach, B, n, ws, raw=False):
    o = _bufs(B, n)
    args = (L.ptr(xd), L.ptr(yd), *_mtl_args(kind, Pd), L.ptr(ld), ALPHA, reach, L.ptr(o["out"]), L.ptr(o["out_a"]), L.ptr(o["out_v"]),
            L.ptr(o["losses"]), L.ptr(o["g_f"]), L.ptr(o["g_a"]), L.ptr(o["g_v"]), L.ptr(o["dfa"]), L.ptr(o["dfv"]), B, n, L.ptr(ws),
            ws.numel(), L.cur_stream())
    if raw:
        return L.load().gdl_head_mtl_ce(*args), o
    L.call("gdl_head_mtl_ce", *args)
    return o


def _three_launch(kind, xd, yd, Pd, ld, reach, B, n):
    """gdl_head_{concat,sum}_fwd + gdl_softmax_ce3(1, alpha, alpha) + gdl_head_{concat,sum}_bwd(out_reaches_xy = reach), dx / dy only"""
    o = _bufs(B, n)
    st = L.cur_stream()
    if kind == "concat":
        L.call("gdl_head_concat_fwd", L.ptr(xd), L.ptr(yd), L.ptr(Pd[0]), L.ptr(Pd[1]), L.ptr(o["out"]), L.ptr(o["out_a"]),
               L.ptr(o["out_v"]), B, n, st)
    else:
        L.call("gdl_head_sum_fwd", L.ptr(xd), L.ptr(yd), L.ptr(Pd[0]), L.ptr(Pd[1]), L.ptr(Pd[2]), L.ptr(Pd[3]), L.ptr(o["out"]),
               L.ptr(o["out_a"]), L.ptr(o["out_v"]), B, n, st)
    L.call("gdl_softmax_ce3", L.ptr(o["out"]), L.ptr(o["out_a"]), L.ptr(o["out_v"]), L.ptr(ld), 1.0, ALPHA, ALPHA, L.ptr(o["losses"]),
           L.ptr(o["g_f"]), L.ptr(o["g_a"]), L.ptr(o["g_v"]), B, n, st)
    if kind == "concat":
        L.call("gdl_head_concat_bwd", L.ptr(xd), L.ptr(yd), L.ptr(Pd[0]), L.ptr(o["g_a"]), L.ptr(o["g_v"]), L.ptr(o["g_f"]), reach, 0,
               L.ptr(o["dfa"]), L.ptr(o["dfv"]), None, None, B, n, st)
    else:
        L.call("gdl_head_sum_bwd", L.ptr(xd), L.ptr(yd), L.ptr(Pd[0]), L.ptr(Pd[2]), L.ptr(o["g_a"]), L.ptr(o["g_v"]), L.ptr(o["g_f"]),
               reach, 0, L.ptr(o["dfa"]), L.ptr(o["dfv"]), None, None, None, None, B, n, st)
    return o


def _ws(B):
    return torch.zeros(L.load().gdl_head_mtl_ce_workspace_bytes(B), dtype=torch.uint8, device=DEV)


# B = 65 and 257: the loss fold's second lane stride (lane l adds b = l and l + 64) and its second lap (b and b + 256)
MTL_SIZES = [(B, n) for B in (1, 5, 16) for n in (1, 6, 34, 309, 512)] + [(65, 6), (257, 6), (257, 34)]


@pytest.mark.parametrize("B,n", MTL_SIZES)
@pytest.mark.parametrize("kind", ["concat", "sum"])
def test_head_mtl_ce(kind, B, n):
    """gdl_head_mtl_ce at one class, fewer classes than waves, a count that is no multiple of the 32-class round over the 16
    waves, the largest dataset and the LDS limit; one sample, an odd batch, 16, and batches that reach the second lane stride and
    the second lap of the loss fold.  Per value of fused_reaches: the logits, the logit
    gradients and dfa / dfv carry the bits of the three-launch path; all of them agree with float64 to rtol 1e-4 / atol 1e-6; each
    loss is within 2 (B - 1) 2^-24 relative of gdl_softmax_ce3's (two float32 summation orders of B non-negative terms); two
    runs on one workspace are bit-equal (the ticket counter comes back at zero)."""
    x, y, P, lab = _head_inputs(kind, B, n)
    xd, yd, Pd, ld = dev(x), dev(y), [dev(p) for p in P], torch.from_numpy(lab).to(DEV)
    ws = _ws(B)
    for reach in (0, 1):
        got = _fused(kind, xd, yd, Pd, ld, reach, B, n, ws)
        again = _fused(kind, xd, yd, Pd, ld, reach, B, n, ws)
        want = _three_launch(kind, xd, yd, Pd, ld, reach, B, n)
        torch.cuda.synchronize()
        ref = ar.head(kind, P, x, y, lab, ALPHA, reach, 0)
        ref["dfa"], ref["dfv"] = ref["dx"], ref["dy"]
        for k in OUTPUTS:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (k, reach)
            assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (k, reach, "second run")
            g = got[k].cpu().numpy()
            err = np.abs(g - ref[k]) / (1e-6 + 1e-4 * np.abs(ref[k]))
            print(kind, B, n, reach, k, "worst error / bound", float(err.max()))
            np.testing.assert_allclose(g, ref[k], rtol=1e-4, atol=1e-6, err_msg=f"{k} reach={reach}")
        assert torch.equal(got["losses"].view(torch.int32), again["losses"].view(torch.int32))
        gl, wl = got["losses"].cpu().numpy().astype(np.float64), want["losses"].cpu().numpy().astype(np.float64)
        print(kind, B, n, reach, "losses", gl, wl)
        assert np.all(np.abs(gl - wl) <= 2 * (B - 1) * 2.0 ** -24 * np.abs(wl)), (gl, wl)
        np.testing.assert_allclose(gl, [ref["loss_f"], ref["loss_a"], ref["loss_v"]], rtol=1e-4, atol=1e-6)
    assert int(ws[:4].view(torch.int32).item()) == 0


def test_head_mtl_ce_refuses_513_classes():
    """n = 513: GDL_ERR_ARG, nothing launched -- the NaN-prefilled outputs stay untouched."""
    B, n = 4, 513
    x, y, P, lab = _head_inputs("concat", B, n)
    rc, o = _fused("concat", dev(x), dev(y), [dev(p) for p in P], torch.from_numpy(lab).to(DEV), 1, B, n, _ws(B), raw=True)
    torch.cuda.synchronize()
    assert rc == 1 and "512 classes" in L.last_error()  # GDL_ERR_ARG
    assert all(bool(torch.isnan(t).all()) for t in o.values())


@pytest.mark.parametrize("bad", [-1, 6])
def test_head_mtl_ce_label_out_of_range(bad):
    """One label outside [0, n): NaN losses (as gdl_softmax_ce), no out-of-bounds access, no one-hot term -- every feature gradient
    stays finite and keeps the three-launch path's bits."""
    B, n = 5, 6
    x, y, P, lab = _head_inputs("sum", B, n)
    lab = lab.copy()
    lab[2] = bad
    xd, yd, Pd, ld = dev(x), dev(y), [dev(p) for p in P], torch.from_numpy(lab).to(DEV)
    got = _fused("sum", xd, yd, Pd, ld, 1, B, n, _ws(B))
    want = _three_launch("sum", xd, yd, Pd, ld, 1, B, n)
    torch.cuda.synchronize()
    assert bool(torch.isnan(got["losses"]).all()) and bool(torch.isnan(want["losses"]).all())
    for k in OUTPUTS:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    others = [b for b in range(B) if b != 2]
    good = lab.copy()
    good[2] = 0
    ref = ar.head("sum", P, x, y, good, ALPHA, 1, 0)
    np.testing.assert_allclose(got["dfa"].cpu().numpy()[others], ref["dx"][others], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got["dfv"].cpu().numpy()[others], ref["dy"][others], rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------ the step
_STATE = {}
_TINY = dict(dataset="CREMAD", n_classes=6, spec_hw=[65, 47], frames=2, image_hw=[64, 64], batch=4, seed=0, lr=2e-3, alpha=ALPHA)


def _state(n_classes, fusion):
    """the seeded initial state (134 M values for the FiLM head): generated once, shared, never modified"""
    if (n_classes, fusion) not in _STATE:
        P, Bf = fx.model_state(n_classes, fusion + "_dgl")
        _STATE[(n_classes, fusion)] = {k: torch.from_numpy(np.array(v)) for k, v in {**P, **Bf}.items()}
    return _STATE[(n_classes, fusion)]


def _make_model(cfg, dtype):
    from models.basic_model import AVClassifier_DGL

    args = argparse.Namespace(fusion_method=cfg["fusion"], dataset=cfg["dataset"], modality="full", batch_size=cfg["batch"])
    model = AVClassifier_DGL(args)
    model.load_state_dict(_state(cfg["n_classes"], cfg["fusion"]), strict=True)
    model = model.to(DEV)
    model.audio_net.gdl_dtype = dtype
    model.visual_net.gdl_dtype = dtype
    return model.train()


def _batch(cfg, st):
    spec, image, label = fx.make_batch(cfg["seed"] + st, cfg["batch"], cfg["spec_hw"], cfg["frames"], cfg["image_hw"],
                                       cfg["n_classes"])
    return dev(spec), dev(image), torch.from_numpy(label).to(DEV)


def _trainer(fusion, dtype="f32", **kw):
    from gdl.trainer import DGLTrainer

    cfg = dict(_TINY, fusion=fusion)
    model = _make_model(cfg, dtype)
    return cfg, model, DGLTrainer(model, lr=cfg["lr"], alpha=cfg["alpha"], **kw)


STEP_FIXTURES = ["abl_concat_nodrop_tiny_b4", "abl_gated_nodrop_tiny_b4", "abl_film_nodrop_tiny_b4", "mtl_concat_tiny_b4",
                 "mtl_sum_tiny_b4", "abl_concat_nodetach_tiny_b4"]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", STEP_FIXTURES)
def test_ablation_step_golden(name, dtype):
    """DGLTrainer under the two switches against the reference's step (make_golden_ablation.py), with the constants
    test_joint_gpu.py::test_joint_step_golden uses for the same quantities at the same shapes.  The fixture's total norm is the
    float64 norm of the reference's float32 gradients and its per-tensor norms are unclipped; the runner reports clipped ones."""
    from gdl.trainer import DGLTrainer

    g = _gold(name)
    cfg = json.loads(str(g["config"]))
    model = _make_model(cfg, dtype)
    head0 = {k: v.detach().clone() for k, v in model.fusion_module.named_parameters()}
    tr = DGLTrainer(model, lr=cfg["lr"], alpha=cfg["alpha"], detach_fused=cfg["detach_fused"], drop_head_uni=cfg["drop_head_uni"])
    f32 = dtype == "f32"
    for st in range(cfg["steps"]):
        spec, image, label = _batch(cfg, st)
        tr.step(spec, image, label)
        r = tr.read()
        pre = f"s{st}."
        later = st > 0
        if later and not f32:
            assert all(np.isfinite(r[k]).all() for k in ("out", "out_a", "out_v")) and np.isfinite(r["total_norm"])
            continue
        lt = (1e-2 if later else 5e-4) if f32 else 0.2
        ls = lt if f32 else 5e-2
        print(name, dtype, st, "logits", max(float(np.abs(r[k] - g[pre + k]).max()) for k in ("out", "out_a", "out_v")), "losses",
              [(r[k], float(g[pre + k])) for k in ("loss_f", "loss_a", "loss_v")], "total_norm", r["total_norm"],
              float(g[pre + "total_norm"]))
        for k in ("out", "out_a", "out_v"):
            np.testing.assert_allclose(r[k], g[pre + k], rtol=lt, atol=lt, err_msg=k)
        for k in ("loss_f", "loss_a", "loss_v"):
            np.testing.assert_allclose(r[k], g[pre + k], rtol=ls, atol=ls, err_msg=k)
        nt = (2e-2 if later else 3e-3) if f32 else 4e-2
        tn = float(g[pre + "total_norm"])
        np.testing.assert_allclose(r["total_norm"], tn, rtol=nt)
        np.testing.assert_allclose(r["audio_grad_sum"], g[pre + "audio_grad_sum"], rtol=2 * nt)
        np.testing.assert_allclose(r["visual_grad_sum"], g[pre + "visual_grad_sum"], rtol=2 * nt)
        names = [str(n) for n in g[pre + "grad_names"]]
        gt = (6e-2 if later else 1e-2) if f32 else 0.3
        clip = min(1.0, 40.0 / (tn + 1e-6))
        worst = 0.0
        for i, n in enumerate(names):
            if g[pre + "grad_is_none"][i]:
                assert n not in r["grad_norm"]  # fc_auxi is outside the optimised arena
                continue
            want = float(g[pre + "grad_norm"][i]) * clip
            worst = max(worst, abs(r["grad_norm"][n] - want) / (want + 1e-30))
            assert abs(r["grad_norm"][n] - want) <= gt * want + 1e-5 * clip * tn, (n, r["grad_norm"][n], want)
        print(name, dtype, st, "worst per-tensor norm deviation", worst)
    last = f"s{cfg['steps'] - 1}."
    names = [str(n) for n in g[last + "grad_names"]]
    ps = g[last + "param_sums"]
    sd = model.state_dict()
    for i, n in enumerate(names):
        got = sd[n].double().abs().sum().item()
        np.testing.assert_allclose(got, ps[i][1], rtol=(2e-5 if cfg["steps"] == 1 else 1e-3) if f32 else 2e-3, err_msg=n)
    if cfg["fusion"] == "concat":  # no loss reaches fc_auxi under any switch: bit-unchanged
        for k in ("fc_auxi.weight", "fc_auxi.bias"):
            assert torch.equal(sd["fusion_module." + k], head0[k]), k
            assert "fusion_module." + k not in tr.names
    if cfg["fusion"] == "gated":  # fc_x / fc_y are trained once the unimodal losses' head gradients are kept
        assert tr.names[:6] == ["fusion_module." + k for k in head0]
        for k in ("fc_x.weight", "fc_x.bias", "fc_y.weight", "fc_y.bias"):
            assert not torch.equal(sd["fusion_module." + k], head0[k]), k
    for k in [k[len(last + "buf."):] for k in g.files if k.startswith(last + "buf.")]:
        tolr, tola = (2e-3, 1e-4) if f32 else (5e-2, 3e-2)
        if cfg["steps"] > 1:
            tola = max(tola, 1e-3)
        np.testing.assert_allclose(sd[k].cpu().numpy().astype(np.float64), g[last + "buf." + k], rtol=tolr, atol=tola, err_msg=k)
    model.eval()
    spec, image, label = _batch(cfg, 1000)
    with torch.no_grad():
        ev = model(spec.unsqueeze(1), image)
    et = (1e-2 if cfg["steps"] > 1 else 2e-3) if f32 else 0.2
    np.testing.assert_allclose(ev[0].cpu().numpy(), g["eval.out"], rtol=et, atol=et)
    # valid() is as in DGL mode: the arg-max of the three eval-mode logit sets, counted on the device
    acc = tr.valid([(spec, image, label)])
    lab = label.cpu().numpy()
    for a, o in zip(acc, ev):
        assert abs(a - float((np.argmax(o.cpu().numpy(), axis=1) == lab).mean())) < 1e-12


def _run_steps(fusion, steps=2, dtype="f32", **kw):
    """(parameters, read()) after `steps` steps of a fresh trainer on the tiny configuration"""
    cfg, model, tr = _trainer(fusion, dtype, **kw)
    for st in range(steps):
        spec, image, label = _batch(cfg, st)
        tr.step(spec, image, label)
    r = tr.read()
    return tr, r


def _flat(tr, r):
    d = {"params": tr.params.cpu().numpy(), "out": r["out"], "out_a": r["out_a"], "out_v": r["out_v"],
         "scalars": np.array([r["loss_f"], r["loss_a"], r["loss_v"], r["total_norm"], r["clip_coef"], r["audio_grad_sum"],
                              r["visual_grad_sum"]], dtype=np.float64),
         "grad_norm": np.array([r["grad_norm"][n] for n in tr.names], dtype=np.float64)}
    return d


def _dump_mtl(fusion, path):
    """(run in a child process, see test_fused_junction_equals_three_launch)"""
    tr, r = _run_steps(fusion, detach_fused=False, drop_head_uni=False)
    np.savez(path, mtl_fused=np.int8(tr.mtl_fused), **_flat(tr, r))


_CHILD = """
import sys
for p in ({tests!r}, {root!r}, {pkg!r}):
    sys.path.insert(0, p)
import test_ablation_gpu as t
t._dump_mtl(sys.argv[1], sys.argv[2])
"""


@pytest.mark.parametrize("fusion", ["concat", "sum"])
def test_fused_junction_equals_three_launch(fusion, tmp_path):
    """The multi-task step with gdl_head_mtl_ce at the junction against the same step with the three launches it replaces (the
    tuning aid GDL_TUNING=1 GDL_MTL_FUSED=0, read once per trainer: a fresh child process): parameters and read() after two steps,
    bit for bit."""
    tr, r = _run_steps(fusion, detach_fused=False, drop_head_uni=False)
    assert tr.mtl_fused
    mine = _flat(tr, r)
    f = str(tmp_path / "three.npz")
    env = dict(os.environ, GDL_TUNING="1", GDL_MTL_FUSED="0")
    c = subprocess.run([sys.executable, "-c", _CHILD.format(tests=HERE, root=ROOT, pkg=os.path.join(ROOT, "iccv2025-gdl_amd")), fusion, f],
                       env=env, capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-2000:]
    other = np.load(f)
    assert int(other["mtl_fused"]) == 0  # the child did take the three-launch path
    for k, v in mine.items():
        assert np.array_equal(v.view(np.int32 if v.dtype == np.float32 else np.int64),
                              other[k].view(np.int32 if v.dtype == np.float32 else np.int64)), (k, v, other[k])


def test_tuning_aid_needs_gdl_tuning(monkeypatch):
    """GDL_MTL_FUSED=0 without GDL_TUNING=1 is ignored, like every tuning aid."""
    monkeypatch.delenv("GDL_TUNING", raising=False)
    monkeypatch.setenv("GDL_MTL_FUSED", "0")
    _, _, tr = _trainer("concat", detach_fused=False, drop_head_uni=False)
    assert tr.mtl_fused


@pytest.mark.parametrize("fusion", ["concat", "gated"])
def test_default_switches_change_nothing(fusion):
    """detach_fused=True, drop_head_uni=True is DGL: parameters and results after two steps are bit-equal to a trainer constructed
    without the keywords, and the checkpoint carries no new key."""
    a, ra = _run_steps(fusion)
    b, rb = _run_steps(fusion, detach_fused=True, drop_head_uni=True)
    assert a.names == b.names and not b.ablation
    fa, fb = _flat(a, ra), _flat(b, rb)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    assert "detach_fused" not in b.state_dict() and "drop_head_uni" not in b.state_dict()


@pytest.mark.parametrize("fusion", ["concat", "sum"])
def test_nodrop_early_backward_identical(fusion):
    """detach_fused=True, drop_head_uni=False keeps the early-backward form (an encoder still learns from its own loss alone;
    only the head backward's flag changes): early backward on and off are bit-equal, and the head does learn something else
    than under DGL."""
    a, ra = _run_steps(fusion, drop_head_uni=False, early_backward=True)
    b, rb = _run_steps(fusion, drop_head_uni=False, early_backward=False)
    fa, fb = _flat(a, ra), _flat(b, rb)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    d, _ = _run_steps(fusion)
    assert not torch.equal(a.params[:a.offsets[a.nf]], d.params[:d.offsets[d.nf]])


def test_checkpoint_records_the_switches():
    """state_dict() round-trips the switches; loading into a trainer with other switches raises, both ways."""
    _, _, t0 = _trainer("concat", detach_fused=False, drop_head_uni=False)
    sd = t0.state_dict()
    assert sd["detach_fused"] is False and sd["drop_head_uni"] is False
    _, _, t1 = _trainer("concat", detach_fused=False, drop_head_uni=False)
    t1.load_state_dict(sd)
    assert (t1.detach_fused, t1.drop_head_uni) == (False, False)
    for kw in (dict(), dict(drop_head_uni=False), dict(detach_fused=False)):
        _, _, other = _trainer("concat", **kw)
        with pytest.raises(L.GdlError, match="detach_fused=False, drop_head_uni=False"):
            other.load_state_dict(sd)
    _, _, plain = _trainer("concat")
    with pytest.raises(L.GdlError, match="detach_fused=True, drop_head_uni=True"):
        t1.load_state_dict(plain.state_dict())


def test_checkpoint_gated_nodrop_resumes_bit_equal():
    """A gated trainer with drop_head_uni=False (six head tensors in the arena) resumed from a checkpoint continues bit-identically."""
    cfg, m0, t0 = _trainer("gated", drop_head_uni=False)
    b0, b1 = _batch(cfg, 0), _batch(cfg, 1)
    t0.step(*b0)
    ck_model = {k: v.clone() for k, v in m0.state_dict().items()}
    ck = t0.state_dict()
    assert ck["steps"] == 1 and ck["drop_head_uni"] is False and ck["detach_fused"] is True
    assert ck["names"][:6] == ["fusion_module." + k for k in ("fc_x.weight", "fc_x.bias", "fc_y.weight", "fc_y.bias", "fc_out.weight",
                                                               "fc_out.bias")]
    t0.step(*b1)
    want = t0.read()
    from gdl.trainer import DGLTrainer

    m1 = _make_model(cfg, "f32")
    m1.load_state_dict(ck_model)
    t1 = DGLTrainer(m1, lr=cfg["lr"], alpha=cfg["alpha"], drop_head_uni=False)
    t1.load_state_dict(ck)
    assert t1.steps == 1
    t1.step(*b1)
    got = t1.read()
    for k in ("out", "out_a", "out_v"):
        np.testing.assert_array_equal(got[k], want[k])
    assert got["total_norm"] == want["total_norm"] and got["loss_f"] == want["loss_f"] and got["loss_a"] == want["loss_a"]
    for k, v in m0.state_dict().items():
        assert torch.equal(v, m1.state_dict()[k]), k


def test_refusals():
    """Everything the switches are not built for is refused with its reason, never ignored."""
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier, AVClassifier_DGL, AVClassifier_DGL_Swin

    def dgl(fusion):
        return AVClassifier_DGL(argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality="full", batch_size=4)).to(DEV)

    concat = dgl("concat")
    joint = AVClassifier(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=4)).to(DEV)
    for kw in (dict(detach_fused=False), dict(drop_head_uni=False), dict(detach_fused=False, drop_head_uni=False)):
        with pytest.raises(L.GdlError, match="truncations of the DGL step"):
            DGLTrainer(joint, lr=1e-3, mode="joint", **kw)
        with pytest.raises(L.GdlError, match="process group"):
            DGLTrainer(concat, lr=1e-3, process_group=object(), **kw)
    sc = fx.SWIN_TINY2
    swin = AVClassifier_DGL_Swin(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", pe=0),
                                 swin_kwargs=dict(img_size=sc["img"], patch_size=sc["patch"], embed_dim=sc["embed"],
                                                  depths=list(sc["depths"]), num_heads=list(sc["heads"]), window_size=sc["window"],
                                                  mlp_ratio=float(sc["mlp"]), drop_path_rate=0.)).to(DEV)
    for kw in (dict(detach_fused=False), dict(drop_head_uni=False)):
        with pytest.raises(L.GdlError, match="Swin"):
            DGLTrainer(swin, lr=1e-3, **kw)
    for fusion in ("gated", "film"):
        m = dgl(fusion)
        for drop in (True, False):
            with pytest.raises(L.GdlError, match=f"concat and sum heads, not for '{fusion}'"):
                DGLTrainer(m, lr=1e-3, detach_fused=False, drop_head_uni=drop)
        del m
