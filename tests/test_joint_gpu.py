"""GPU tests of the joint-training baselines (BASELINE config 1: ONE cross-entropy on the fused logits, the gradient flowing
through the head into both encoders) for the sum, gated and FiLM heads: the head entry points of the C ABI against the
reference's goldens and against float64 restatements, the joint forward against the DGL forward, DGLTrainer(mode="joint")
against the step goldens (tests/golden/make_golden_joint.py), the drop-in autograd path against the runner, valid(),
checkpoints, and the refusals that stay."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import head_ref as R
from oracle import fixtures as fx

pytestmark = pytest.mark.gpu

from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEAD_NAMES = {
    "sum": ("fc_x.weight", "fc_x.bias", "fc_y.weight", "fc_y.bias"),
    "gated": ("fc_x.weight", "fc_x.bias", "fc_y.weight", "fc_y.bias", "fc_out.weight", "fc_out.bias"),
    "film": ("fc.weight", "fc.bias", "fc_out.weight", "fc_out.bias"),
}


def _head_shapes(kind, n):
    return {"sum": ((n, 512), (n,), (n, 512), (n,)),
            "gated": ((512, 512), (512,), (512, 512), (512,), (n, 512), (n,)),
            "film": ((512, 512 * 512), (512,), (n, 512), (n,))}[kind]


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


# ------------------------------------------------------------------ the head entry points
def _joint_fwd(kind, P, x, y, x_gate=True):
    """`out` of the jointly trained head through the C ABI + what its backward needs."""
    B, n = x.shape[0], P[-1].shape[0]
    out = torch.empty(B, n, device=DEV)
    s = L.cur_stream()
    if kind == "sum":
        L.call("gdl_head_sum_fwd", L.ptr(x), L.ptr(y), L.ptr(P[0]), L.ptr(P[1]), L.ptr(P[2]), L.ptr(P[3]), L.ptr(out), None, None,
               B, n, s)
        return out, ()
    if kind == "gated":
        hx, hy = torch.empty(B, 512, device=DEV), torch.empty(B, 512, device=DEV)
        L.call("gdl_head_gated_joint_fwd", L.ptr(x), L.ptr(y), *(L.ptr(p) for p in P), L.ptr(hx), L.ptr(hy), L.ptr(out),
               int(x_gate), B, n, s)
        return out, (hx, hy)
    nb = L.load().gdl_head_film_workspace_bytes(B)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    hidden = torch.empty(B, 512, device=DEV)
    L.call("gdl_head_film_joint_fwd", L.ptr(x), L.ptr(y), *(L.ptr(p) for p in P), L.ptr(hidden), L.ptr(out), B, n, L.ptr(ws), nb, s)
    return out, (hidden, ws)


def _joint_bwd(kind, P, x, y, saved, go, x_gate=True, keep=None):
    """(dx, dy, [parameter gradients in named_parameters() order]) from g_out; keep (a dict): the gated head's ws goes there."""
    B, n = x.shape[0], P[-1].shape[0]
    dx, dy = torch.full_like(x, float("nan")), torch.full_like(y, float("nan"))
    G = [torch.full_like(p, float("nan")) for p in P]
    s = L.cur_stream()
    if kind == "sum":
        L.call("gdl_head_sum_bwd", L.ptr(x), L.ptr(y), L.ptr(P[0]), L.ptr(P[2]), None, None, L.ptr(go), 1, 0, L.ptr(dx), L.ptr(dy),
               *(L.ptr(g) for g in G), B, n, s)
    elif kind == "gated":
        hx, hy = saved
        ws = torch.empty(2 * B * 512, device=DEV)
        L.call("gdl_head_gated_joint_bwd", L.ptr(x), L.ptr(y), L.ptr(hx), L.ptr(hy), L.ptr(P[0]), L.ptr(P[2]), L.ptr(P[4]), L.ptr(go),
               int(x_gate), L.ptr(dx), L.ptr(dy), *(L.ptr(g) for g in G), L.ptr(ws), B, n, s)
        if keep is not None:
            keep["ws"] = ws
    else:
        hidden, ws = saved
        L.call("gdl_head_film_joint_bwd", L.ptr(x), L.ptr(y), L.ptr(P[0]), L.ptr(P[2]), L.ptr(hidden), L.ptr(go), L.ptr(dx), L.ptr(dy),
               *(L.ptr(g) for g in G), B, n, L.ptr(ws), ws.numel(), s)
    torch.cuda.synchronize()
    return dx, dy, G


@pytest.mark.parametrize("name,kind,x_gate", [("head_sum_c6", "sum", True), ("head_gated_c6", "gated", True),
                                              ("head_gated_ygate_c6", "gated", False), ("head_film_c6", "film", True)])
def test_joint_head_golden(name, kind, x_gate):
    """Each jointly trained head through the C ABI against the reference's golden (fusion_modules.py:5-13, 181-210, 91-124):
    forward `out`, then every backward output.  Tolerances of the DGL test of the same head (tests/test_step_gpu.py)."""
    g = _gold(name)
    n = 6
    assert bool(g["x_gate"]) == x_gate
    st = fx.make_state({"fusion_module." + k: sh for k, sh in zip(HEAD_NAMES[kind], _head_shapes(kind, n))})
    P = [dev(st["fusion_module." + k]) for k in HEAD_NAMES[kind]]
    x, y, go = dev(g["x"]), dev(g["y"]), dev(g["g_out"])
    # (rtol, atol of the logits, atol of the gradients) of test_head_sum_dgl_golden / _gated_ / _film_
    tol, atol_out, atol = {"sum": (2e-4, 2e-5, 1e-4), "gated": (2e-4, 1e-4, 2e-4), "film": (1e-3, 1e-3, 1e-3)}[kind]
    out, saved = _joint_fwd(kind, P, x, y, x_gate)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), g["out"], rtol=tol, atol=atol_out)
    dx, dy, G = _joint_bwd(kind, P, x, y, saved, go, x_gate)

    def close(got, key):
        got = got.cpu().numpy()
        if key in g.files:
            np.testing.assert_allclose(got, g[key], rtol=tol, atol=atol, err_msg=key)
        else:
            step = 9973 if got.size > 10 ** 7 else 97
            np.testing.assert_allclose(np.sqrt((got.astype(np.float64) ** 2).sum()), float(g[key + ".norm"]), rtol=tol, err_msg=key)
            np.testing.assert_allclose(got.reshape(-1)[::step], g[key + ".sample97"], rtol=tol, atol=atol, err_msg=key)

    close(dx, "dx")
    close(dy, "dy")
    for k, t in zip(HEAD_NAMES[kind], G):
        close(t, "grad." + k)


def _check64(got, ref, key):
    """the bounds of test_head_film_beyond_64_samples: element-wise 1e-3 / 1e-3 on logits and feature gradients"""
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-3, atol=1e-3, err_msg=key)


def _check64_param(got, ref, key):
    """... and 1e-3 of the largest element (+ 1e-6) on parameter gradients"""
    scale = float(ref.abs().max())
    assert float((got.double() - ref).abs().max()) <= 1e-3 * scale + 1e-6, key


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, device=DEV)


def _bound64(got, ref, key):
    """within the derived bound of tests/head_ref.py, element by element"""
    ex = R.excess(got.cpu().numpy(), ref[0], ref[1])
    print(key, "excess", ex)
    assert ex <= 1.0, (key, "is", ex, "bounds from the float64 value")


@pytest.mark.parametrize("B,n", [(5, 6), (33, 34)])
@pytest.mark.parametrize("kind,x_gate", [("sum", True), ("gated", True), ("gated", False)])
def test_joint_head_float64(kind, x_gate, B, n):
    """The sum and gated joint heads against the float64 restatements of tests/head_ref.py, every element within the bound derived
    there, at a batch that is no multiple of anything and one beyond a 32-sample group, with more classes than a block has waves.
    Sum: the whole forward and backward (each output is one sum deep).  Gated: stage by stage, each stage restated from the
    device's own output of the stage before (hx / hy, the halves of ws).  The end-to-end comparison this test made before (1e-3 /
    1e-3 on logits and feature gradients, 1e-3 of the largest element + 1e-6 on parameter gradients) stays beside them."""
    gen = torch.Generator(device=DEV).manual_seed(100 * B + n)
    P = [_randn(gen, *sh) * (0.05 if len(sh) == 2 else 0.1) for sh in _head_shapes(kind, n)]
    x, y = _randn(gen, B, 512).clamp_min(0), _randn(gen, B, 512).clamp_min(0)
    go = _randn(gen, B, n) / B
    out, saved = _joint_fwd(kind, P, x, y, x_gate)
    keep = {}
    dx, dy, G = _joint_bwd(kind, P, x, y, saved, go, x_gate, keep)
    Pn = [p.cpu().numpy() for p in P]
    xn, yn, gn = x.cpu().numpy(), y.cpu().numpy(), go.cpu().numpy()
    if kind == "sum":
        f = R.lin_fwd(R.F64, "sum", xn, yn, Pn[0], Pn[1], Pn[2], Pn[3])
        b = R.lin_bwd(R.F64, "sum", xn, yn, Pn[0], Pn[2], None, None, gn, 1, 0)
        _bound64(out, f["out"], "out")
        _bound64(dx, b["dx"], "dx")
        _bound64(dy, b["dy"], "dy")
        for k, t, r in zip(HEAD_NAMES[kind], G, ("dWx", "dbx", "dWy", "dby")):
            _bound64(t, b[r], k)
        D = [p.double() for p in P]
        xd, yd, gd = x.double(), y.double(), go.double()
        _check64(out, xd @ D[0].T + D[1] + yd @ D[2].T + D[3], "out")
        _check64(dx, gd @ D[0], "dx")
        _check64(dy, gd @ D[2], "dy")
        for k, t, r in zip(HEAD_NAMES[kind], G, [gd.T @ xd, gd.sum(0), gd.T @ yd, gd.sum(0)]):
            _check64_param(t, r, k)
        return
    hxn, hyn = saved[0].cpu().numpy(), saved[1].cpu().numpy()
    h = R.gated_hidden(R.F64, xn, yn, Pn[0], Pn[1], Pn[2], Pn[3])
    _bound64(saved[0], h["hx"], "hx")
    _bound64(saved[1], h["hy"], "hy")
    assert max(np.abs(hxn).max(), np.abs(hyn).max()) <= R.H_MAX
    _bound64(out, R.gated_joint_logits(R.F64, hxn, hyn, Pn[4], Pn[5], x_gate)["out"], "out")
    ws = keep["ws"].cpu().numpy()
    dhx, dhy = ws[:B * 512].reshape(B, 512), ws[B * 512:].reshape(B, 512)
    rd = R.gated_joint_dh(R.F64, hxn, hyn, Pn[4], gn, x_gate)
    _bound64(keep["ws"][:B * 512].view(B, 512), rd["dhx"], "dhx")
    _bound64(keep["ws"][B * 512:].view(B, 512), rd["dhy"], "dhy")
    r = R.gated_dx(R.F64, dhx, dhy, Pn[0], Pn[2])
    _bound64(dx, r["dx"], "dx")
    _bound64(dy, r["dy"], "dy")
    r = R.gated_dw1(R.F64, dhx, dhy, xn, yn)
    gate, val = (hxn, hyn) if x_gate else (hyn, hxn)
    r.update(R.gated_dwo(R.F64, gate, val, None, None, gn, 0))
    for k, t, rk in zip(HEAD_NAMES[kind], G, ("dW1", "db1", "dW2", "db2", "dWo", "dbo")):
        _bound64(t, r[rk], k)
    # end to end, as before
    D = [p.double() for p in P]
    xd, yd, gd = x.double(), y.double(), go.double()
    hx, hy = xd @ D[0].T + D[1], yd @ D[2].T + D[3]
    gate, val = (hx, hy) if x_gate else (hy, hx)
    s = torch.sigmoid(gate)
    m = s * val
    ref_out = m @ D[4].T + D[5]
    dm = gd @ D[4]
    dval, dgate = dm * s, dm * val * s * (1 - s)
    dhx, dhy = (dgate, dval) if x_gate else (dval, dgate)
    rdx, rdy = dhx @ D[0], dhy @ D[2]
    Rp = [dhx.T @ xd, dhx.sum(0), dhy.T @ yd, dhy.sum(0), gd.T @ m, gd.sum(0)]
    _check64(out, ref_out, "out")
    _check64(dx, rdx, "dx")
    _check64(dy, rdy, "dy")
    for k, t, r in zip(HEAD_NAMES[kind], G, Rp):
        _check64_param(t, r, k)


_FILM = {}


def _film_params(n=6):
    """FiLM parameters at the scale of test_head_film_beyond_64_samples, made once on the device and left unchanged."""
    if n not in _FILM:
        gen = torch.Generator(device=DEV).manual_seed(7)
        _FILM[n] = [_randn(gen, 512, 512 * 512) * 2e-3, _randn(gen, 512) * 0.1, _randn(gen, n, 512) * 0.05, _randn(gen, n) * 0.1]
    return _FILM[n]


@pytest.mark.parametrize("B", [5, 33, 65])
def test_joint_film_float64(B):
    """The FiLM joint head against float64 (torch, on the device) at B = 5 (one padded column block), 33 (batch padding to 32
    for the weight gradient, 64 for T) and 65 (a second 64-sample group in film_h_kernel / film_joint_dxy_kernel)."""
    n = 6
    P = _film_params(n)
    gen = torch.Generator(device=DEV).manual_seed(B)
    x, y = _randn(gen, B, 512).clamp_min(0), _randn(gen, B, 512).clamp_min(0)
    go = _randn(gen, B, n) / B
    out, saved = _joint_fwd("film", P, x, y)
    dx, dy, G = _joint_bwd("film", P, x, y, saved, go)
    A = P[0].double().view(512 * 512, 512)  # row (k, i), column j
    xd, yd, gd = x.double(), y.double(), go.double()
    T3 = (A @ yd.T).view(512, 512, B)  # [k][i][b] = (W_k y_b)[i]
    h = torch.einsum("bi,kib->bk", xd, T3) + P[1].double()
    _check64(out, h @ P[2].double().T + P[3].double(), "out")
    _check64(saved[0], h, "hidden")
    dh = gd @ P[2].double()
    _check64(dx, torch.einsum("bk,kib->bi", dh, T3), "dx")
    del T3
    U = torch.einsum("bk,bi->kib", dh, xd).reshape(512 * 512, B)
    _check64(dy, U.T @ A, "dy")
    _check64_param(G[0].view(512 * 512, 512), U @ yd, "fc.weight")
    _check64_param(G[1], dh.sum(0), "fc.bias")
    _check64_param(G[2], gd.T @ h, "fc_out.weight")
    _check64_param(G[3], gd.sum(0), "fc_out.bias")


@pytest.mark.parametrize("kind,B", [("sum", 33), ("gated", 33), ("film", 5), ("film", 64)])
def test_joint_forward_equals_dgl_forward(kind, B):
    """`out` of the joint forward is bit-identical to `out` of the DGL forward of the same head on the same inputs: the
    detach changes no value (film at 64: the joint head contracts 64 columns of T where the DGL head contracts 128)."""
    n = 6
    gen = torch.Generator(device=DEV).manual_seed(B)
    if kind == "film":
        P = _film_params(n)
    else:
        P = [_randn(gen, *sh) * (0.05 if len(sh) == 2 else 0.1) for sh in _head_shapes(kind, n)]
    x, y = _randn(gen, B, 512).clamp_min(0), _randn(gen, B, 512).clamp_min(0)
    out, _ = _joint_fwd(kind, P, x, y, True)
    ref, xo, yo = (torch.empty(B, n, device=DEV) for _ in range(3))
    s = L.cur_stream()
    if kind == "sum":
        L.call("gdl_head_sum_fwd", L.ptr(x), L.ptr(y), *(L.ptr(p) for p in P), L.ptr(ref), L.ptr(xo), L.ptr(yo), B, n, s)
    elif kind == "gated":
        hx, hy = torch.empty(B, 512, device=DEV), torch.empty(B, 512, device=DEV)
        L.call("gdl_head_gated_fwd", L.ptr(x), L.ptr(y), *(L.ptr(p) for p in P), L.ptr(hx), L.ptr(hy), L.ptr(ref), L.ptr(xo),
               L.ptr(yo), B, n, s)
    else:
        nb = L.load().gdl_head_film_workspace_bytes(B)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        hidden = torch.empty(3, B, 512, device=DEV)
        L.call("gdl_head_film_fwd", L.ptr(x), L.ptr(y), *(L.ptr(p) for p in P), L.ptr(hidden), L.ptr(ref), L.ptr(xo), L.ptr(yo), B, n,
               L.ptr(ws), nb, s)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


# ------------------------------------------------------------------ the joint step
_STATE = {}


def _state(n_classes, fusion):
    """the seeded initial state (134 M values for the FiLM head): generated once, shared, never modified"""
    if (n_classes, fusion) not in _STATE:
        P, Bf = fx.model_state(n_classes, fusion + "_dgl")  # the joint heads have their DGL twins' parameter sets
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
    return model


def _batch(cfg, st):
    spec, image, label = fx.make_batch(cfg["seed"] + st, cfg["batch"], cfg["spec_hw"], cfg["frames"], cfg["image_hw"],
                                       cfg["n_classes"])
    return dev(spec), dev(image), torch.from_numpy(label).to(DEV)


_TINY = dict(dataset="CREMAD", n_classes=6, spec_hw=[65, 47], frames=2, image_hw=[64, 64], batch=4, seed=0, lr=2e-3)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["joint_sum_tiny_b4", "joint_gated_tiny_b4", "joint_film_tiny_b4"])
def test_joint_step_golden(name, dtype):
    """DGLTrainer(mode="joint") against the reference's single-loss step, with the constants test_native_step_golden uses for
    the DGL fixture of the same head (tiny shapes).  The fixture's total norm is the float64 norm of the reference's float32
    gradients and its per-tensor norms are unclipped (make_golden_joint.py); the runner reports clipped ones."""
    from gdl.trainer import DGLTrainer

    g = _gold(name)
    cfg = json.loads(str(g["config"]))
    model = _make_model(cfg, dtype)
    model.train()
    P0 = {k: v.detach().clone() for k, v in model.fusion_module.named_parameters()}
    tr = DGLTrainer(model, lr=cfg["lr"], mode="joint")
    assert tr.names[:len(P0)] == ["fusion_module." + k for k in P0]  # every head tensor is in the arena
    f32 = dtype == "f32"
    for st in range(cfg["steps"]):
        spec, image, label = _batch(cfg, st)
        tr.step(spec, image, label)
        r = tr.read()
        pre = f"s{st}."
        later = st > 0
        assert "out_a" not in r and "out_v" not in r
        if later and not f32:
            assert np.isfinite(r["out"]).all() and np.isfinite(r["total_norm"])
            continue
        lt = (1e-2 if later else 5e-4) if f32 else 0.2
        ls = lt if f32 else 5e-2
        print(name, dtype, st, "logits", float(np.abs(r["out"] - g[pre + "out"]).max()), "loss", r["loss_f"], float(g[pre + "loss_f"]),
              "total_norm", r["total_norm"], float(g[pre + "total_norm"]))
        np.testing.assert_allclose(r["out"], g[pre + "out"], rtol=lt, atol=lt)
        np.testing.assert_allclose(r["loss_f"], g[pre + "loss_f"], rtol=ls, atol=ls)
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
            want = float(g[pre + "grad_norm"][i]) * clip
            worst = max(worst, abs(r["grad_norm"][n] - want) / (want + 1e-30))
            assert abs(r["grad_norm"][n] - want) <= gt * want + 1e-5 * clip * tn, (n, r["grad_norm"][n], want)
        print(name, dtype, st, "worst per-tensor norm deviation", worst)
    if cfg["fusion"] == "gated":  # fc_x / fc_y are trained by the joint loss (they are not in DGL mode)
        for k in ("fc_x.weight", "fc_x.bias", "fc_y.weight", "fc_y.bias"):
            assert "fusion_module." + k in tr.names
            assert not torch.equal(dict(model.fusion_module.named_parameters())[k].detach(), P0[k]), k
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
        ev = model(spec.unsqueeze(1), image)[2]
    et = (1e-2 if cfg["steps"] > 1 else 2e-3) if f32 else 0.2
    np.testing.assert_allclose(ev.cpu().numpy(), g["eval.out"], rtol=et, atol=et)


@pytest.mark.parametrize("fusion", ["sum", "gated", "film"])
def test_dropin_joint_step_equals_runner(fusion):
    """The script-style body on the mirror module -- model(...), one CrossEntropyLoss, backward, clip_grad_norm_, optim.SGD --
    against DGLTrainer(mode="joint") on the same state and batch, to the bounds test_dropin_autograd_step_golden holds the
    drop-in path to (logits / loss 5e-4, norms 3e-3, mean-|g| sums 6e-3, parameter sums after the update 2e-5)."""
    import torch.nn as nn

    from gdl.trainer import DGLTrainer

    cfg = dict(_TINY, fusion=fusion)
    spec, image, label = _batch(cfg, 0)
    model = _make_model(cfg, "f32")
    optimizer = torch.optim.SGD(model.parameters(), lr=cfg["lr"], momentum=0.9, weight_decay=1e-4)
    criterion = nn.CrossEntropyLoss()
    model.train()
    optimizer.zero_grad()
    _, _, out = model(spec.unsqueeze(1).float(), image.float())
    loss = criterion(out, label)
    loss.backward()
    assert all(p.grad is not None for p in model.parameters())
    norms = {n: p.grad.double().norm().item() for n, p in model.named_parameters()}  # before the clip
    total = nn.utils.clip_grad_norm_(model.parameters(), max_norm=40, norm_type=2).item()
    a_sum = sum(torch.abs(p.grad).mean().item() for p in model.audio_net.parameters())
    v_sum = sum(torch.abs(p.grad).mean().item() for p in model.visual_net.parameters())
    optimizer.step()
    want_out, want_loss = out.detach().cpu().numpy(), loss.item()
    want_sums = {k: v.double().abs().sum().item() for k, v in model.state_dict().items()}
    del model, optimizer, out, loss
    m2 = _make_model(cfg, "f32")
    m2.train()
    tr = DGLTrainer(m2, lr=cfg["lr"], mode="joint")
    tr.step(spec, image, label)
    r = tr.read()
    np.testing.assert_allclose(r["out"], want_out, rtol=5e-4, atol=5e-4)
    np.testing.assert_allclose(r["loss_f"], want_loss, rtol=5e-4)
    np.testing.assert_allclose(r["total_norm"], total, rtol=3e-3)
    np.testing.assert_allclose(r["audio_grad_sum"], a_sum, rtol=6e-3)
    np.testing.assert_allclose(r["visual_grad_sum"], v_sum, rtol=6e-3)
    clip = min(1.0, 40.0 / (total + 1e-6))
    for n, v in norms.items():
        assert abs(r["grad_norm"][n] - v * clip) <= 3e-3 * v * clip + 1e-5 * clip * total, (n, r["grad_norm"][n], v * clip)
    for k, v in m2.state_dict().items():
        np.testing.assert_allclose(v.double().abs().sum().item(), want_sums[k], rtol=2e-5, atol=1e-6, err_msg=k)


@pytest.mark.parametrize("fusion", ["sum", "gated", "film"])
def test_valid_joint(fusion):
    """valid() in joint mode on two tiny batches equals arg-max counting of the eval-mode logits on the host."""
    from gdl.trainer import DGLTrainer

    cfg = dict(_TINY, fusion=fusion)
    model = _make_model(cfg, "f32")
    tr = DGLTrainer(model, lr=cfg["lr"], mode="joint")
    batches = [_batch(cfg, 1000), _batch(cfg, 1001)]
    acc = tr.valid(batches)
    model.eval()
    hit = tot = 0
    num = np.zeros(cfg["n_classes"])
    with torch.no_grad():
        for spec, image, label in batches:
            o = model(spec.unsqueeze(1), image)[2].cpu().numpy()
            lab = label.cpu().numpy()
            hit += int((np.argmax(o, axis=1) == lab).sum())
            tot += len(lab)
            num += np.bincount(lab, minlength=cfg["n_classes"])
    assert abs(acc[0] - hit / tot) < 1e-12 and acc[1] == 0.0 and acc[2] == 0.0
    np.testing.assert_array_equal(tr.valid_counts[0], num)


def test_joint_checkpoint_gated():
    """state_dict() / load_state_dict() of a gated joint trainer (six head tensors in the arena): a run resumed from the
    checkpoint continues bit-identically."""
    from gdl.trainer import DGLTrainer

    cfg = dict(_TINY, fusion="gated")

    def fresh():
        m = _make_model(cfg, "f32")
        m.train()
        return m, DGLTrainer(m, lr=cfg["lr"], mode="joint")

    m0, t0 = fresh()
    b0, b1 = _batch(cfg, 0), _batch(cfg, 1)
    t0.step(*b0)
    ck_model = {k: v.clone() for k, v in m0.state_dict().items()}
    ck_opt = t0.state_dict()
    assert ck_opt["steps"] == 1 and ck_opt["names"][:6] == ["fusion_module." + k for k in HEAD_NAMES["gated"]]
    t0.step(*b1)
    want = t0.read()
    m1, _ = fresh()
    m1.load_state_dict(ck_model)
    t1 = DGLTrainer(m1, lr=cfg["lr"], mode="joint")  # (re-alias the arena to the loaded weights)
    t1.load_state_dict(ck_opt)
    assert t1.steps == 1
    t1.step(*b1)
    got = t1.read()
    np.testing.assert_array_equal(got["out"], want["out"])
    assert got["total_norm"] == want["total_norm"] and got["loss_f"] == want["loss_f"]
    for k, v in m0.state_dict().items():
        assert torch.equal(v, m1.state_dict()[k]), k


def test_refusals_stay():
    """The Swin composition stays DGL + concat only, also under the new mode name; GatedFusion_DGL stays x_gate=True only."""
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier_DGL_Swin
    from models.fusion_modules import GatedFusion_DGL

    sc = fx.SWIN_TINY2
    args = argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", pe=0)
    model = AVClassifier_DGL_Swin(args, swin_kwargs=dict(img_size=sc["img"], patch_size=sc["patch"], embed_dim=sc["embed"],
                                                         depths=list(sc["depths"]), num_heads=list(sc["heads"]),
                                                         window_size=sc["window"], mlp_ratio=float(sc["mlp"]),
                                                         drop_path_rate=0.)).to(DEV)
    for mode in ("joint", "concat"):
        with pytest.raises(L.GdlError, match="Swin"):
            DGLTrainer(model, lr=1e-3, mode=mode)
    with pytest.raises(NotImplementedError):
        GatedFusion_DGL(output_dim=6, x_gate=False)
