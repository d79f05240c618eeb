"""GPU tests of the MMPareto integration: gdl_pareto_integrate against the float64 restatement (tests/pareto_ref.py) with bounds
derived from the number formats, at every alignment of both pointers; the guard the step rests on -- gdl_encoder_backward may be
repeated for one training forward; DGLTrainer(pareto=True) against the step goldens (tests/golden/make_golden_pareto.py), against
the plain multi-task step where the two must agree bit for bit, against itself, across a checkpoint; the refusals."""
import argparse
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pareto_ref as pr  # noqa: E402
import test_ablation_gpu as ta  # noqa: E402  (the tiny configuration, its models and batches: shared, not copied)
from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev  # noqa: E402

U = pr.U
CANARY = 12345.6789  # what stands around g_m and g_u in their buffers
PAD = 16  # floats in front of the vector: 64 bytes, so `PAD + off` is `off` floats past a 16-byte boundary


# ------------------------------------------------------------------ gdl_pareto_integrate
def _place(v, off):
    """a device buffer [canary x (PAD + off) | v | canary x (PAD + 3)] and the offset of v in it (the allocation is 256-byte
    aligned: v starts `off` floats behind a 16-byte boundary)"""
    buf = torch.full((PAD + off + v.size + PAD + 3,), CANARY, device=DEV)
    assert buf.data_ptr() % 256 == 0
    buf[PAD + off:PAD + off + v.size] = torch.from_numpy(v).to(DEV)
    return buf, PAD + off


def _integrate(g_m, g_u, scale=1.0, off_m=0, off_u=0, stream=None):
    """One call; returns (out, info[8], (c_m, c_u)) after checking that nothing but g_m's n elements was written."""
    n = g_m.size
    bm, sm = _place(g_m, off_m)
    bu, su = _place(g_u, off_u)
    bu0 = bu.clone()
    info = torch.full((8,), float("nan"), device=DEV)
    nb = L.load().gdl_pareto_workspace_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    st = stream if stream is not None else torch.cuda.current_stream()
    L.call("gdl_pareto_integrate", bm.data_ptr() + 4 * sm, bu.data_ptr() + 4 * su, n, scale, L.ptr(info), L.ptr(ws), nb, st.cuda_stream)
    st.synchronize()
    can = torch.tensor(CANARY, device=DEV)
    assert bool((bm[:sm] == can).all()) and bool((bm[sm + n:] == can).all()), "a canary around g_m changed"
    assert torch.equal(bu.view(torch.int32), bu0.view(torch.int32)), "g_u (or a canary around it) changed"
    return bm[sm:sm + n].cpu().numpy(), info.cpu().numpy(), ws[:8].view(torch.float32).cpu().numpy()


def _random_pair(n, mix, ratio, seed):
    """float32 vectors of cosine about `mix` and norm ratio about `ratio`, redrawn (deterministically) until
    |S_mu| >= 1e-3 sum |g_m g_u|: the branch then does not hang on the rounding of a sum"""
    for k in range(200):
        rs = np.random.default_rng([11, n, seed, k])
        a, b = rs.standard_normal(n), rs.standard_normal(n)
        g_m = a.astype(np.float32)
        g_u = (ratio * (mix * a + np.sqrt(1.0 - mix * mix) * b)).astype(np.float32)
        p = g_m.astype(np.float64) * g_u.astype(np.float64)
        if abs(p.sum()) >= 1e-3 * np.abs(p).sum() and np.abs(p).sum() > 0:
            return g_m, g_u
    raise AssertionError("no well-conditioned draw")


def _case(kind, n):
    rs = np.random.default_rng([13, n])
    x = rs.standard_normal(n).astype(np.float32)
    if kind == "interior":
        return _random_pair(n, 0.3, 1.2, 0)
    if kind == "conflict":  # S_mu < 0
        g_m, g_u = _random_pair(n, 0.6, 0.8, 1)
        g_u = -g_u if np.dot(g_m.astype(np.float64), g_u.astype(np.float64)) > 0 else g_u
        return g_m, g_u
    if kind == "gm_is_3gu":
        return np.float32(3) * x, x
    if kind == "gu_is_3gm":
        return x, np.float32(3) * x
    if kind == "disjoint":  # S_mu == 0 exactly
        even = (np.arange(n) % 2 == 0)
        return np.where(even, x, 0).astype(np.float32), np.where(even, 0, x).astype(np.float32)
    if kind == "equal":  # D == 0
        return x, x.copy()
    if kind == "gu_zero":
        return x, np.zeros(n, np.float32)
    if kind == "both_zero":
        return np.zeros(n, np.float32), np.zeros(n, np.float32)
    if kind == "nan":
        g_u = rs.standard_normal(n).astype(np.float32)
        g_u[n // 2] = np.nan
        return x, g_u
    raise KeyError(kind)


KINDS = ["interior", "conflict", "gm_is_3gu", "gu_is_3gm", "disjoint", "equal", "gu_zero", "both_zero", "nan"]
SIZES = [1, 3, 5, 4097, 8191, 262147]  # one element .. one block with a ragged end .. 32 whole blocks of 8192 and three elements
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 3), (1, 2), (3, 0)]  # (g_m, g_u) floats past a 16-byte boundary


def _check(kind, g_m, g_u, out, info, coef, scale=1.0):
    """One result against the restatement.  Bounds (u = 2^-24):
      S_*                  2 u relative: the double sums differ from the restatement's by n 2^-53 relative to sum |terms|, which
                           the conditioning of the draw keeps below 1e3 n 2^-53 of the sum itself; the rest is ONE rounding to float
      gamma, w_m, w_u, s   4 u relative: the same, and one rounding to float
      g[i]                 4 u (|c_m g_m[i]| + |c_u g_u[i]|) of c_u g_u[i] + c_m g_m[i] evaluated in float64 with the device's own
                           c_m, c_u: one rounding of the product, one of the fused multiply-add
    The device's c_m, c_u are the float roundings of scale s w in double: within 4 u of the restatement's."""
    c = pr.coefficients(*pr.sums(g_m, g_u), scale=scale)
    assert int(info[7]) == c["branch"], (info, c)
    finite = np.isfinite(c["S_mm"]) and np.isfinite(c["S_uu"]) and np.isfinite(c["S_mu"])
    worst = {}
    if finite:
        for i, k in enumerate(pr.INFO_KEYS[:7]):
            tol = (2 if i < 3 else 4) * U * abs(c[k])
            worst[k] = abs(float(info[i]) - c[k]) / (abs(c[k]) + 1e-300)
            assert abs(float(info[i]) - c[k]) <= tol, (k, float(info[i]), c[k])
    else:
        assert tuple(info[3:7]) == (0.5, 1.0, 1.0, 1.0)
    for got, k in zip(coef, ("c_m", "c_u")):
        assert abs(float(got) - c[k]) <= 4 * U * abs(c[k]), (k, float(got), c[k])
    want = pr.combine(g_m, g_u, coef[0], coef[1])
    bound = 4 * U * (np.abs(float(coef[0]) * g_m.astype(np.float64)) + np.abs(float(coef[1]) * g_u.astype(np.float64)))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out), nan)
    err = np.abs(out.astype(np.float64) - want)[~nan]
    assert np.all(err <= bound[~nan]), (kind, float((err / (bound[~nan] + 1e-300)).max()))
    worst["g / bound"] = float((err / (bound[~nan] + 1e-300)).max()) if err.size else 0.0
    return c, worst


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_pareto_integrate(kind, n):
    """Every case at every size, g_m and g_u at every offset from a 16-byte boundary: the canaries around g_m and all of g_u are
    unchanged (checked in `_integrate`), info / the coefficients / the output meet `_check`'s bounds, and the offsets do not enter
    -- every placement gives the bytes of the first."""
    g_m, g_u = _case(kind, n)
    if kind in ("interior", "conflict"):  # the condition the draw was made for, asserted on the host before the call
        p = g_m.astype(np.float64) * g_u.astype(np.float64)
        assert abs(p.sum()) >= 1e-3 * np.abs(p).sum()
    first = None
    for off_m, off_u in OFFSETS:
        out, info, coef = _integrate(g_m, g_u, off_m=off_m, off_u=off_u)
        c, worst = _check(kind, g_m, g_u, out, info, coef)
        if first is None:
            first = (out, info, coef)
            print(kind, n, "branch", c["branch"], "gamma", c["gamma"], "s", c["s"], "worst deviations", worst)
        else:
            for a, b in zip(first, (out, info, coef)):
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (off_m, off_u)
    out, info, coef = first
    c = pr.coefficients(*pr.sums(g_m, g_u))
    if kind == "interior" and n >= 4097:
        assert c["branch"] == 1 and 0.05 < c["gamma"] < 0.95
    if kind == "conflict":
        assert c["branch"] == 0 and c["S_mu"] < 0 and np.array_equal(out, g_m + g_u)
    if kind == "gm_is_3gu":
        assert c["branch"] == 1 and info[3] == 0.0 and info[4] == 0.0 and info[5] == 2.0
        np.testing.assert_allclose(out, g_m.astype(np.float64) + g_u, rtol=8 * U, atol=0)
    if kind == "gu_is_3gm":
        assert c["branch"] == 1 and info[3] == 1.0 and info[4] == 2.0 and info[5] == 0.0
        np.testing.assert_allclose(out, g_m.astype(np.float64) + g_u, rtol=8 * U, atol=0)
    if kind == "disjoint":
        assert info[2] == 0.0 and c["branch"] == 0 and info[6] == 1.0 and np.array_equal(out, g_m + g_u)
    if kind == "equal":
        assert tuple(info[3:8]) == (0.5, 1.0, 1.0, 1.0, 1.0) and np.array_equal(out, np.float32(2) * g_m)
    if kind == "gu_zero":
        assert c["branch"] == 0 and info[6] == 1.0 and np.array_equal(out, g_m)
    if kind == "both_zero":
        assert c["branch"] == 0 and info[6] == 1.0 and not out.any()
    if kind == "nan":
        keep = np.arange(n) != n // 2
        assert c["branch"] == 0 and info[6] == 1.0 and np.isnan(out[n // 2]) and np.array_equal(out[keep], (g_m + g_u)[keep])


def test_pareto_integrate_scale_and_the_folds_second_lap():
    """pareto_scale enters the coefficients alone; n = 257 blocks of 8192 and five elements: the fold of the blocks' sums takes its
    second lap (sum t adds blocks t and t + 256)."""
    g_m, g_u = _random_pair(4097, 0.3, 1.2, 5)
    out, info, coef = _integrate(g_m, g_u, scale=0.375, off_m=1, off_u=2)
    _check("interior", g_m, g_u, out, info, coef, scale=0.375)
    _, info1, coef1 = _integrate(g_m, g_u, off_m=1, off_u=2)
    assert np.array_equal(info, info1) and abs(coef[0] - 0.375 * coef1[0]) <= 2 * U * abs(coef[0])
    n = 257 * 8192 + 5
    g_m, g_u = _random_pair(n, 0.3, 1.2, 6)
    out, info, coef = _integrate(g_m, g_u, off_m=3, off_u=1)
    c, worst = _check("interior", g_m, g_u, out, info, coef)
    print("n", n, "worst deviations", worst)
    assert c["branch"] == 1


@pytest.mark.parametrize("n", [5, 8191, 262147])
def test_pareto_integrate_repeats_bit_for_bit(n):
    """Two calls on the same input give identical bytes; a call on another stream with other pointer offsets gives identical info
    (and output): no sum depends on the stream, the grid or the alignment."""
    g_m, g_u = _case("interior", n)
    a = _integrate(g_m, g_u, off_m=2, off_u=1)
    b = _integrate(g_m, g_u, off_m=2, off_u=1)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        c = _integrate(g_m, g_u, off_m=1, off_u=3, stream=side)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
        assert np.array_equal(x.view(np.int32), z.view(np.int32))


def test_pareto_integrate_refuses():
    """n <= 0, a NULL pointer, a workspace too small: GDL_ERR_ARG, nothing launched -- the prefilled buffers keep their bits."""
    lib = L.load()
    g = torch.full((64,), CANARY, device=DEV)
    h = torch.full((64,), CANARY, device=DEV)
    info = torch.full((8,), CANARY, device=DEV)
    nb = lib.gdl_pareto_workspace_bytes(64)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    st = L.cur_stream()
    assert lib.gdl_pareto_workspace_bytes(0) == 0 and lib.gdl_pareto_workspace_bytes(-3) == 0 and nb > 0
    for args in ((L.ptr(g), L.ptr(h), 0), (L.ptr(g), L.ptr(h), -1), (None, L.ptr(h), 64), (L.ptr(g), None, 64)):
        assert lib.gdl_pareto_integrate(*args, 1.0, L.ptr(info), L.ptr(ws), nb, st) == 1  # GDL_ERR_ARG
    assert lib.gdl_pareto_integrate(L.ptr(g), L.ptr(h), 64, 1.0, None, L.ptr(ws), nb, st) == 1
    assert lib.gdl_pareto_integrate(L.ptr(g), L.ptr(h), 64, 1.0, L.ptr(info), None, nb, st) == 1
    assert lib.gdl_pareto_integrate(L.ptr(g), L.ptr(h), 64, 1.0, L.ptr(info), L.ptr(ws), nb - 1, st) == 1
    assert "workspace" in L.last_error()
    torch.cuda.synchronize()
    can = torch.tensor(CANARY, device=DEV)
    assert bool((g == can).all()) and bool((h == can).all()) and bool((info == can).all()) and not bool(ws.any())


# ------------------------------------------------------------------ the engine: two backwards of one forward
def _engine(modality, dtype, net, B, T, H, W):
    from gdl.encoder import EncoderEngine

    eng = EncoderEngine(modality, dtype, B, T, H, W, DEV)
    bns = net._bn_layers()
    eng.set_params([p.data for p in net.engine_parameters()], [b.running_mean for b in bns], [b.running_var for b in bns],
                   [b.num_batches_tracked for b in bns])
    return eng


def _grads(net):
    return [torch.full_like(p.data, float("nan")) for p in net.engine_parameters()]


# the tiny shapes of the step tests, and one bf16 visual shape wide enough (128 columns) for the fused stem backward
ENGINE_CASES = [("audio", "f32", None), ("audio", "bf16", None), ("visual", "f32", None), ("visual", "bf16", None),
                ("visual", "bf16", (1, 1, 128, 128))]


@pytest.mark.parametrize("modality,dtype,shape", ENGINE_CASES)
def test_encoder_backward_may_be_repeated(modality, dtype, shape):
    """One training forward, then backward from dfeat into G1 and the same backward into G2: all 60 tensors byte-equal.  Then
    backward from another dfeat2 into G3: byte-equal to a FRESH engine's forward + backward from dfeat2 on the same parameters
    and input -- the first two backwards consumed nothing of what the forward kept."""
    cfg = dict(ta._TINY, fusion="concat")
    model = ta._make_model(cfg, dtype)
    net = model.audio_net if modality == "audio" else model.visual_net
    B = cfg["batch"]
    if shape is None:
        shape = (B, 1, *cfg["spec_hw"]) if modality == "audio" else (B, cfg["frames"], *cfg["image_hw"])
    B, T, H, W = shape
    rs = np.random.default_rng([17, modality == "audio", H])
    x = dev(rs.standard_normal((B, 1 if modality == "audio" else 3, T, H, W), dtype=np.float32))
    df1 = dev(rs.standard_normal((B, 512), dtype=np.float32) * 1e-2)
    df2 = dev(rs.standard_normal((B, 512), dtype=np.float32) * 1e-2)
    eng = _engine(modality, dtype, net, B, T, H, W)
    G1, G2, G3, G4 = _grads(net), _grads(net), _grads(net), _grads(net)
    eng.forward(x, True)
    eng.backward(G1, dfeat=df1)
    eng.backward(G2, dfeat=df1)
    eng.backward(G3, dfeat=df2)
    fresh = _engine(modality, dtype, net, B, T, H, W)
    fresh.forward(x, True)
    fresh.backward(G4, dfeat=df2)
    torch.cuda.synchronize()
    assert len(G1) == 60
    for i, (a, b, c, d) in enumerate(zip(G1, G2, G3, G4)):
        assert bool(torch.isfinite(a).all()), i
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ("the repeated backward differs", i)
        assert torch.equal(c.view(torch.int32), d.view(torch.int32)), ("the third backward differs from a fresh engine's", i)
    assert any(not torch.equal(a, c) for a, c in zip(G1, G3))  # (dfeat2 is another gradient)


# ------------------------------------------------------------------ the step
GOLDENS = ["pareto_concat_tiny_b4", "pareto_sum_tiny_b4", "pareto_concat_a1_tiny_b4"]  # the last: alpha = 1.0, an interior gamma


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", GOLDENS)
def test_pareto_step_golden(name, dtype):
    """DGLTrainer(pareto=True) against the literal torch loop on the reference's encoders (make_golden_pareto.py), two steps, with
    the constants test_ablation_gpu.py::test_ablation_step_golden uses for the same quantities at the same shapes (f32 and bf16).
    read()["pareto"]: the branch is the golden's; in f32 gamma and s are held to that test's norm tolerance `nt`."""
    from gdl.trainer import DGLTrainer

    g = ta._gold(name)
    cfg = json.loads(str(g["config"]))
    model = ta._make_model(cfg, dtype)
    head0 = {k: v.detach().clone() for k, v in model.fusion_module.named_parameters()}
    tr = DGLTrainer(model, lr=cfg["lr"], alpha=cfg["alpha"], detach_fused=False, drop_head_uni=False, pareto=True,
                    pareto_scale=cfg["pareto_scale"])
    f32 = dtype == "f32"
    for st in range(cfg["steps"]):
        spec, image, label = ta._batch(cfg, st)
        tr.step(spec, image, label)
        r = tr.read()
        pre = f"s{st}."
        later = st > 0
        for e in ("audio", "visual"):
            want = dict(zip(pr.INFO_KEYS, g[pre + f"pareto.{e}"]))
            got = r["pareto"][e]
            print(name, dtype, st, e, "pareto", got, "golden gamma", want["gamma"], "s", want["s"], "branch", int(want["branch"]))
            assert got["branch"] == int(want["branch"]), (e, got, want)  # at every (dtype, step)
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
        if f32:
            for e in ("audio", "visual"):
                want = dict(zip(pr.INFO_KEYS, g[pre + f"pareto.{e}"]))
                np.testing.assert_allclose(r["pareto"][e]["gamma"], want["gamma"], rtol=nt, err_msg=e + " gamma")
                np.testing.assert_allclose(r["pareto"][e]["s"], want["s"], rtol=nt, err_msg=e + " s")
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
    if cfg["fusion"] == "concat":  # no loss reaches fc_auxi: bit-unchanged
        for k in ("fc_auxi.weight", "fc_auxi.bias"):
            assert torch.equal(sd["fusion_module." + k], head0[k]), k
    for k in [k[len(last + "buf."):] for k in g.files if k.startswith(last + "buf.")]:
        tolr, tola = (2e-3, 1e-4) if f32 else (5e-2, 3e-2)
        if cfg["steps"] > 1:
            tola = max(tola, 1e-3)
        np.testing.assert_allclose(sd[k].cpu().numpy().astype(np.float64), g[last + "buf." + k], rtol=tolr, atol=tola, err_msg=k)
    model.eval()
    spec, image, label = ta._batch(cfg, 1000)
    with torch.no_grad():
        ev = model(spec.unsqueeze(1), image)
    et = (1e-2 if cfg["steps"] > 1 else 2e-3) if f32 else 0.2
    np.testing.assert_allclose(ev[0].cpu().numpy(), g["eval.out"], rtol=et, atol=et)


def _gold_cfg(fusion):
    return json.loads(str(ta._gold(f"pareto_{fusion}_tiny_b4")["config"]))


def _run(fusion, steps, dtype="f32", **kw):
    from gdl.trainer import DGLTrainer

    cfg = _gold_cfg(fusion)
    model = ta._make_model(cfg, dtype)
    tr = DGLTrainer(model, lr=cfg["lr"], alpha=cfg["alpha"], detach_fused=False, drop_head_uni=False, **kw)
    for st in range(steps):
        tr.step(*ta._batch(cfg, st))
    return cfg, model, tr, tr.read()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("fusion", ["concat", "sum"])
def test_pareto_step0_forward_is_the_multitask_steps(fusion, dtype):
    """Step 0 from the same state: the pareto step and the plain multi-task step give bit-equal out, out_a, out_v, losses and
    BatchNorm buffers (one forward each; the second backward re-runs nothing of it) -- and another gradient for the encoders."""
    _, ma_, ta_, ra = _run(fusion, 1, dtype)
    _, mb_, tb_, rb = _run(fusion, 1, dtype, pareto=True)
    for k in ("out", "out_a", "out_v"):
        assert np.array_equal(ra[k].view(np.int32), rb[k].view(np.int32)), k
    for k in ("loss_f", "loss_a", "loss_v"):
        assert ra[k] == rb[k], k
    for (k, a), (_, b) in zip(ma_.named_buffers(), mb_.named_buffers()):
        assert torch.equal(a, b), k
    nf = ta_.offsets[ta_.nf]
    assert not torch.equal(ta_.params[nf:], tb_.params[nf:])
    assert "pareto" not in ra and set(rb["pareto"]) == {"audio", "visual"}
    # the head takes the plain multi-task gradient: its tensors' norms differ by the two steps' clip coefficients alone (read()
    # reports clipped norms as float32: 4 roundings of 2^-24 each side)
    for n in ta_.names[:ta_.nf]:
        a, b = ra["grad_norm"][n] / ra["clip_coef"], rb["grad_norm"][n] / rb["clip_coef"]
        assert abs(a - b) <= 8 * U * abs(a), (n, a, b)


def test_pareto_two_runs_are_byte_identical():
    _, _, t0, r0 = _run("concat", 2, pareto=True)
    _, _, t1, r1 = _run("concat", 2, pareto=True)
    assert torch.equal(t0.params.view(torch.int32), t1.params.view(torch.int32))
    assert r0["pareto"] == r1["pareto"] and r0["total_norm"] == r1["total_norm"]


def test_pareto_checkpoint_resumes_bit_equal():
    """A checkpoint taken after step 1 resumes bit-equal; it records the switch, and loading it into a trainer without pareto --
    or a plain checkpoint into a pareto trainer -- raises."""
    from gdl.trainer import DGLTrainer

    cfg = _gold_cfg("sum")
    kw = dict(lr=cfg["lr"], alpha=cfg["alpha"], detach_fused=False, drop_head_uni=False)
    m0 = ta._make_model(cfg, "f32")
    t0 = DGLTrainer(m0, pareto=True, pareto_scale=0.5, **kw)
    b0, b1 = ta._batch(cfg, 0), ta._batch(cfg, 1)
    t0.step(*b0)
    ck_model = {k: v.clone() for k, v in m0.state_dict().items()}
    ck = t0.state_dict()
    assert ck["steps"] == 1 and ck["pareto"] is True and ck["pareto_scale"] == 0.5
    t0.step(*b1)
    want = t0.read()
    m1 = ta._make_model(cfg, "f32")
    m1.load_state_dict(ck_model)
    t1 = DGLTrainer(m1, pareto=True, pareto_scale=0.5, **kw)
    t1.load_state_dict(ck)
    t1.step(*b1)
    got = t1.read()
    for k in ("out", "out_a", "out_v"):
        np.testing.assert_array_equal(got[k], want[k])
    assert got["total_norm"] == want["total_norm"] and got["pareto"] == want["pareto"]
    for k, v in m0.state_dict().items():
        assert torch.equal(v, m1.state_dict()[k]), k
    other = DGLTrainer(ta._make_model(cfg, "f32"), pareto=True, pareto_scale=1.0, **kw)
    with pytest.raises(L.GdlError, match=r"trained with pareto_scale=0\.5, this trainer runs pareto_scale=1\.0"):
        other.load_state_dict(ck)
    plain = DGLTrainer(ta._make_model(cfg, "f32"), **kw)
    assert "pareto" not in plain.state_dict()
    with pytest.raises(L.GdlError, match="with pareto integration, this trainer runs without"):
        plain.load_state_dict(ck)
    with pytest.raises(L.GdlError, match="without pareto integration, this trainer runs with"):
        t1.load_state_dict(plain.state_dict())


def test_pareto_refusals():
    """Everything the integration is not built for is refused with its reason, never ignored."""
    from gdl.prototypes import Prototypes
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier, AVClassifier_DGL, AVClassifier_DGL_Swin
    from oracle import fixtures as fx

    def ns(fusion, **kw):
        return argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality="full", batch_size=4, **kw)

    mtl = dict(lr=1e-3, detach_fused=False, drop_head_uni=False, pareto=True)
    concat = AVClassifier_DGL(ns("concat")).to(DEV)
    joint = AVClassifier(ns("concat")).to(DEV)
    with pytest.raises(L.GdlError, match="pareto=True .*the 'joint' step has one loss"):
        DGLTrainer(joint, lr=1e-3, mode="joint", pareto=True)
    for kw in (dict(), dict(detach_fused=False), dict(drop_head_uni=False)):
        with pytest.raises(L.GdlError, match="pareto=True needs both DGL truncations lifted"):
            DGLTrainer(concat, lr=1e-3, pareto=True, **kw)
    with pytest.raises(L.GdlError, match="pareto=True with a process group"):
        DGLTrainer(concat, process_group=object(), **mtl)
    with pytest.raises(L.GdlError, match="pareto=True with beta"):
        DGLTrainer(concat, beta=0.5, **mtl)
    with pytest.raises(L.GdlError, match="pareto=True with prototypes"):
        DGLTrainer(concat, prototypes=Prototypes(6, DEV), **mtl)
    for mod in ("OGM", "OGM_GE"):
        with pytest.raises(L.GdlError, match=f"pareto=True with modulation='{mod}'"):
            DGLTrainer(concat, modulation=mod, **mtl)
    with pytest.raises(ValueError, match="pareto_scale"):
        DGLTrainer(concat, pareto_scale=float("inf"), **mtl)
    for fusion in ("gated", "film"):
        m = AVClassifier_DGL(ns(fusion)).to(DEV)
        with pytest.raises(L.GdlError, match=f"pareto=True is built for the concat and sum heads, not for '{fusion}'"):
            DGLTrainer(m, **mtl)
        del m
    wide = AVClassifier_DGL(ns("concat")).to(DEV)  # a 513-class concat head: one class beyond gdl_head_mtl_ce
    wide.fusion_module.fc_out = torch.nn.Linear(1024, 513).to(DEV)
    with pytest.raises(L.GdlError, match="pareto=True handles at most 512 classes .*the head has 513"):
        DGLTrainer(wide, **mtl)
    del wide
    sc = fx.SWIN_TINY2
    swin = AVClassifier_DGL_Swin(ns("concat", pe=0),
                                 swin_kwargs=dict(img_size=sc["img"], patch_size=sc["patch"], embed_dim=sc["embed"],
                                                  depths=list(sc["depths"]), num_heads=list(sc["heads"]), window_size=sc["window"],
                                                  mlp_ratio=float(sc["mlp"]), drop_path_rate=0.)).to(DEV)
    with pytest.raises(L.GdlError, match="pareto=True is not built for the Swin visual branch"):
        DGLTrainer(swin, **mtl)
    pe = AVClassifier_DGL(ns("concat", pe=1)).to(DEV)
    with pytest.raises(L.GdlError, match="pareto=True beside the probabilistic-embedding branch"):
        DGLTrainer(pe, **mtl)
