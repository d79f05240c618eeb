"""CPU-only checks of the linear probe (gdl.probe, csrc/linprobe.hip): the float64 restatement tests/probe_ref.py against the
torch float32 trajectories of the fixtures (tests/golden/make_golden_probe.py), the C ABI, the order-table builder, the
scripts' learning-rate schedule, and everything that is refused on the host."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import probe_ref as R
from gdl import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("gdl_linprobe_workspace_bytes", "gdl_linprobe_epoch")


@pytest.mark.parametrize("name", ["probe_audio_tiny", "probe_visual_tiny"])
def test_restatement_matches_the_torch_trajectories(name):
    """probe_ref.fit (float64) from the fixture's start against the fixture's torch float32 fit, after each of the 3 epochs, at
    max_norm 40 and at the clipping max_norm.  The deviations are the fixtures' own float32 noise: probe_ref.GOLDEN32_DEV
    records their largest values (the GPU test's bounds are multiples of it), so each must stay within it -- 5 % of slack for
    a float64 BLAS that sums in another order."""
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    cfg = json.loads(str(g["config"]))
    assert g["features"].shape == (12, 512) and g["order"].shape == (3, 3, 4) and g["W0"].shape == (6, 512)
    assert not np.array_equal(g["n40.e2.W"], g["clip.e2.W"])
    for run, mn in (("n40", cfg["max_norm"]), ("clip", cfg["clip_norm"])):
        traj = R.fit(g["features"], g["labels"], g["order"], g["W0"], g["b0"], lr=cfg["lr"], mu=cfg["momentum"],
                     wd=cfg["weight_decay"], max_norm=mn)
        norms = np.concatenate([t["norms"] for t in traj])
        assert (norms > mn).all() if run == "clip" else (norms < mn).all()  # the clip run clips at EVERY step
        np.testing.assert_allclose(norms, np.concatenate([g[f"{run}.e{e}.norms"] for e in range(3)]), rtol=1e-5)
        for e, t in enumerate(traj):
            for k in ("W", "b", "mW", "mb"):
                d = R.deviation(g[f"{run}.e{e}.{k}"], t[k])
                assert d <= 1.05 * R.GOLDEN32_DEV[k], (run, e, k, d)
            assert R.loss_deviation(g[f"{run}.e{e}.loss"], t["loss"]) <= 1.05 * R.GOLDEN32_DEV["loss"], (run, e)


def test_restatement_label_out_of_range():
    """No one-hot term and a NaN loss for the sample; the step's update equals the hand-built one."""
    r = np.random.default_rng(3)
    f, W = np.abs(r.standard_normal((3, 512))), 0.05 * r.standard_normal((4, 512))
    b, y = np.zeros(4), np.array([1, 7, -1])
    W1, b1, mW, mb = W.copy(), b.copy(), np.zeros_like(W), np.zeros_like(b)
    loss, _ = R.step(W1, b1, mW, mb, f, y, 0.1, 0.9, 0.0, 1e9)
    assert np.isnan(loss)
    out = f @ W.T
    p = np.exp(out) / np.exp(out).sum(1, keepdims=True)
    p[0, 1] -= 1.0
    np.testing.assert_allclose(W1, W - 0.1 * (p / 3).T @ f, rtol=1e-12, atol=1e-15)


def test_abi_exports_the_probe_entry_points():
    src = open(os.path.join(ROOT, "include", "gdl_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"GDL_API\s+[\w\s\*]+?\b(gdl_\w+)\s*\(", src))
    lib = L.load()
    for name in SYMBOLS:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name)
    assert L.SIGNATURES["gdl_linprobe_workspace_bytes"] == ("z", "ii")
    assert L.SIGNATURES["gdl_linprobe_epoch"] == ("i", "ppl" + "pii" + "pppp" + "i" + "ffff" + "p" + "pz" + "p")
    # the header's parameter list, type by type, against the binding table
    m = re.search(r"gdl_linprobe_epoch\s*\((.*?)\)\s*;", src, flags=re.S)
    code = "".join("p" if "*" in a else {"int": "i", "int64_t": "l", "float": "f", "size_t": "z"}[a.split()[-2]]
                   for a in (x.strip() for x in m.group(1).split(",")))
    assert code == L.SIGNATURES["gdl_linprobe_epoch"][1]
    assert lib.gdl_linprobe_workspace_bytes(64, 6) >= 4 * (64 * 6 + 64 + 6 * 512 + 6) + 8 * 12
    assert lib.gdl_linprobe_workspace_bytes(64, 6) % 16 == 0
    for B, n in ((64, 513), (64, 0), (0, 6)):
        assert lib.gdl_linprobe_workspace_bytes(B, n) == 0
    # argument checks run on the host before any launch
    one = ctypes.c_void_p(256)  # never dereferenced
    args = lambda n=6, B=4, steps=1, N=12: (one, one, N, one, steps, B, one, one, one, one, n, 1e-3, 0.9, 1e-4, 40.0, one, one, 1 << 20, None)  # noqa: E731
    assert lib.gdl_linprobe_epoch(*args(n=513)) == 1 and b"n_classes" in lib.gdl_last_error()
    assert lib.gdl_linprobe_epoch(*args(n=0)) == 1
    assert lib.gdl_linprobe_epoch(*args(B=0)) == 1 and b"B = 0" in lib.gdl_last_error()
    assert lib.gdl_linprobe_epoch(*args(steps=-1)) == 1
    assert lib.gdl_linprobe_epoch(*args(N=0)) == 1
    assert lib.gdl_linprobe_epoch(None, None, 12, None, 0, 4, None, None, None, None, 6, 1e-3, 0.9, 1e-4, 40.0, None, None, 0, None) == 1
    assert b"null" in lib.gdl_last_error()
    small = list(args())
    small[17] = 16
    assert lib.gdl_linprobe_epoch(*small) == 4 and b"workspace" in lib.gdl_last_error()  # GDL_ERR_WORKSPACE


def test_order_table():
    import gdl

    gen = torch.Generator().manual_seed(5)
    tab = gdl.probe_order(70, 3, 4, gen)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (4, 23, 3)  # 70 // 3 steps: the ragged tail (1 row) is dropped
    for e in range(4):
        flat = tab[e].reshape(-1).numpy()
        assert len(set(flat.tolist())) == flat.size == 69 and flat.min() >= 0 and flat.max() < 70  # at most once per epoch
    assert not torch.equal(tab[0], tab[1])
    assert torch.equal(tab, gdl.probe_order(70, 3, 4, torch.Generator().manual_seed(5)))  # the same seed, the same table
    assert not torch.equal(tab, gdl.probe_order(70, 3, 4, torch.Generator().manual_seed(6)))
    # it IS torch.randperm on that generator, cut to whole batches
    g2 = torch.Generator().manual_seed(5)
    assert torch.equal(tab[0].reshape(-1), torch.randperm(70, generator=g2)[:69].to(torch.int32))
    assert tuple(gdl.probe_order(12, 4, 1, gen).shape) == (1, 3, 4)  # B divides N: nothing dropped
    with pytest.raises(L.GdlError, match="batch_size"):
        gdl.probe_order(5, 8, 1, gen)
    # the fixture's table is what a probe seeded 0 draws after its weight
    g = np.load(os.path.join(GOLD, "probe_audio_tiny.npz"), allow_pickle=False)
    g0 = torch.Generator().manual_seed(0)
    w = torch.empty((6, 512)).normal_(0.0, float(np.sqrt(2.0 / (512 + 6))), generator=g0)
    assert np.array_equal(w.numpy(), g["W0"])  # (nn.init.xavier_normal_ in the generator script)
    assert np.array_equal(gdl.probe_order(12, 4, 3, g0).numpy(), g["order"])


@pytest.mark.parametrize("milestones", [[70], [30, 70]])
def test_multistep_lr_is_the_scripts_schedule(milestones):
    """torch's MultiStepLR driven in the scripts' call order: scheduler.step() at the top of train_epoch (main_dgl.py:73-74),
    before the epoch's optimizer steps."""
    import gdl

    lr0, ratio = 1e-3, 0.1
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr0, momentum=0.9)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones, ratio)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (torch warns about step() before optimizer.step(): the scripts' order)
        for epoch in range(100):
            sched.step()
            assert gdl.multistep_lr(lr0, milestones, ratio, epoch) == opt.param_groups[0]["lr"], epoch
            p.grad = torch.zeros(1)
            opt.step()
    m = milestones[0]
    assert gdl.multistep_lr(lr0, milestones, ratio, m - 2) == lr0  # the decay arrives one epoch before the milestone's number
    assert gdl.multistep_lr(lr0, milestones, ratio, m - 1) == lr0 * ratio
    with pytest.raises(ValueError):
        gdl.multistep_lr(lr0, milestones, ratio, -1)


def test_refusals():
    import gdl
    from gdl import probe

    assert gdl.LinearProbe is probe.LinearProbe and gdl.extract_features is probe.extract_features
    assert gdl.FeatureBank is probe.FeatureBank and gdl.multistep_lr is probe.multistep_lr
    with pytest.raises(L.GdlError, match="n_classes"):
        gdl.LinearProbe(513, "cuda:0")  # refused before the device is looked at
    with pytest.raises(L.GdlError, match="n_classes"):
        gdl.LinearProbe(0, "cuda:0")
    with pytest.raises(L.GdlError, match="no CPU path"):
        gdl.LinearProbe(6, "cpu")
    # an order table is checked on the host
    ok = np.arange(12, dtype=np.int64).reshape(1, 3, 4)
    assert probe.check_order(ok, 12, 1, 4).dtype == torch.int32
    for bad in (12, -1):
        t = ok.copy()
        t[0, 1, 2] = bad
        with pytest.raises(L.GdlError, match="outside"):
            probe.check_order(t, 12, 1, 4)
    with pytest.raises(L.GdlError, match="table"):
        probe.check_order(ok, 12, 2, 4)  # epochs
    with pytest.raises(L.GdlError, match="table"):
        probe.check_order(ok.astype(np.float32), 12, 1, 4)
    with pytest.raises(L.GdlError, match="table"):
        probe.check_order(ok.reshape(1, 2, 6), 12, 1, 4)  # batch_size
    # the encoder: Swin is refused with its reason, as are a missing encoder, an unknown modality and a CPU model
    swin = types.SimpleNamespace(audio_net=None, visual_net=types.SimpleNamespace(cfg={}, num_features=768), modality="full")
    with pytest.raises(L.GdlError, match="Swin.*768"):
        gdl.extract_features(swin, "visual", [])
    from models.basic_model import AVClassifier_DGL
    import argparse

    audio = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="audio", batch_size=4))
    with pytest.raises(L.GdlError, match="no visual_net"):
        gdl.extract_features(audio, "visual", [])
    with pytest.raises(L.GdlError, match="modality"):
        gdl.extract_features(audio, "text", [])
    with pytest.raises(L.GdlError, match="cuda"):
        gdl.extract_features(audio, "audio", [])
    with pytest.raises(L.GdlError, match="FeatureBank"):
        gdl.FeatureBank(torch.zeros(3, 768), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(L.GdlError, match="labels"):
        gdl.FeatureBank(torch.zeros(3, 512), torch.zeros(3, dtype=torch.int32))
