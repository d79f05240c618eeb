"""CPU-only checks of the DGL ablation switches and the multi-task baseline: the float64 restatement the GPU tests lean on
(tests/ablation_ref.py) against the head-level fixtures captured from the imported reference (tests/golden/make_golden_ablation.py),
the integrity of the step fixtures, the C ABI's new entry point, and the refusals that need no device."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest

import ablation_ref as ar
from gdl import _lib as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEP_FIXTURES = {  # name: (fusion, detach_fused, drop_head_uni, steps)
    "abl_concat_nodrop_tiny_b4": ("concat", True, False, 2),
    "abl_gated_nodrop_tiny_b4": ("gated", True, False, 2),
    "abl_film_nodrop_tiny_b4": ("film", True, False, 1),
    "mtl_concat_tiny_b4": ("concat", False, False, 2),
    "mtl_sum_tiny_b4": ("sum", False, False, 2),
    "abl_concat_nodetach_tiny_b4": ("concat", False, True, 2),
}
HEAD_PARAMS = {"concat": ("fc_out.weight", "fc_out.bias"), "sum": ("fc_x.weight", "fc_x.bias", "fc_y.weight", "fc_y.bias")}


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def head_params(kind, n):
    """the fixture's head state: fx.make_state of the head's own tensors (fc_auxi included for the concat head, unused)"""
    from oracle import fixtures as fx

    shapes = {"concat": {"fc_out.weight": (n, 1024), "fc_out.bias": (n,), "fc_auxi.weight": (n, 1024), "fc_auxi.bias": (n,)},
              "sum": {"fc_x.weight": (n, 512), "fc_x.bias": (n,), "fc_y.weight": (n, 512), "fc_y.bias": (n,)}}[kind]
    st = fx.make_state({"fusion_module." + k: v for k, v in shapes.items()})
    return [st["fusion_module." + k] for k in HEAD_PARAMS[kind]]


@pytest.mark.parametrize("reach,uni", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("kind", ["concat", "sum"])
def test_ablation_ref_against_head_fixture(kind, reach, uni):
    """The float64 restatement against float32 autograd of the imported head: rtol 1e-4, atol 1e-6, the bound
    test_head_uni_dfeat holds the same quantities to."""
    g = _gold(f"head_mtl_{kind}_c6")
    r = ar.head(kind, head_params(kind, 6), g["x"], g["y"], g["label"], float(g["alpha"]), reach, uni)
    tol = dict(rtol=1e-4, atol=1e-6)
    for k in ("out", "out_a", "out_v", "loss_f", "loss_a", "loss_v"):
        np.testing.assert_allclose(r[k], g[k], err_msg=k, **tol)
    pre = f"r{reach}u{uni}."
    np.testing.assert_allclose(r["dx"], g[pre + "dx"], err_msg="dx", **tol)
    np.testing.assert_allclose(r["dy"], g[pre + "dy"], err_msg="dy", **tol)
    for k, got in zip(HEAD_PARAMS[kind], r["grads"]):
        np.testing.assert_allclose(got, g[pre + "grad." + k], err_msg=k, **tol)
    if kind == "concat":  # fc_auxi never receives a gradient, under any flag
        assert not any("fc_auxi" in f for f in g.files if ".grad." in f)
        assert [str(s) for s in g["param_names"]] == ["fc_out.weight", "fc_out.bias", "fc_auxi.weight", "fc_auxi.bias"]


def test_head_fixture_flags_matter():
    """The fixture separates the four combinations: `reach` changes dx / dy alone, `uni` the parameter gradients alone."""
    for kind in ("concat", "sum"):
        g = _gold(f"head_mtl_{kind}_c6")
        w = HEAD_PARAMS[kind][0]
        assert not np.array_equal(g["r0u0.dx"], g["r1u0.dx"]) and np.array_equal(g["r0u0.dx"], g["r0u1.dx"])
        assert not np.array_equal(g["r0u0.grad." + w], g["r0u1.grad." + w])
        np.testing.assert_allclose(g["r0u0.grad." + w], g["r1u0.grad." + w], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("name", sorted(STEP_FIXTURES))
def test_step_fixture_integrity(name):
    fusion, detach, drop, steps = STEP_FIXTURES[name]
    g = _gold(name)
    cfg = json.loads(str(g["config"]))
    assert (cfg["fusion"], cfg["detach_fused"], cfg["drop_head_uni"], cfg["steps"]) == (fusion, detach, drop, steps)
    assert cfg["alpha"] == 2.5 and cfg["mode"] == "dgl" and cfg["batch"] == 4 and cfg["lr"] == 2e-3
    assert os.path.getsize(os.path.join(GOLD, name + ".npz")) < 1 << 20
    for st in range(steps):
        pre = f"s{st}."
        for k in ("out", "out_a", "out_v", "loss_f", "loss_a", "loss_v", "total_norm", "grad_norm", "grad_is_none", "param_sums"):
            assert pre + k in g.files, k
        names = [str(n) for n in g[pre + "grad_names"]]
        none = [n for n, f in zip(names, g[pre + "grad_is_none"]) if f]
        # fc_auxi is the one tensor no loss reaches; every other tensor is trained
        assert none == (["fusion_module.fc_auxi.weight", "fusion_module.fc_auxi.bias"] if fusion == "concat" else []), none
        gn = dict(zip(names, g[pre + "grad_norm"]))
        assert all(v > 0 for n, v in gn.items() if n not in none)
        if name == "abl_gated_nodrop_tiny_b4":  # the unimodal losses train fc_x / fc_y once their head gradients are kept
            for k in ("fc_x.weight", "fc_x.bias", "fc_y.weight", "fc_y.bias"):
                assert gn["fusion_module." + k] > 0
    assert "eval.out" in g.files


def test_fixtures_differ_where_the_switches_act():
    """Same state, same batch: step 0's logits agree across the concat fixtures (the switches change no forward value), the
    encoder gradients differ once the fused loss reaches them, the head's once the unimodal losses do."""
    a, b, c = _gold("abl_concat_nodrop_tiny_b4"), _gold("mtl_concat_tiny_b4"), _gold("abl_concat_nodetach_tiny_b4")
    for k in ("s0.out", "s0.out_a", "s0.out_v"):
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(b[k], c[k], rtol=1e-5, atol=1e-6)
    names = [str(n) for n in a["s0.grad_names"]]
    i_head, i_enc = names.index("fusion_module.fc_out.weight"), names.index("audio_net.conv1.weight")
    assert abs(a["s0.grad_norm"][i_head] - b["s0.grad_norm"][i_head]) < 1e-4 * a["s0.grad_norm"][i_head]  # both keep the unimodal part
    assert abs(a["s0.grad_norm"][i_enc] - b["s0.grad_norm"][i_enc]) > 1e-3 * a["s0.grad_norm"][i_enc]
    assert abs(c["s0.grad_norm"][i_head] - b["s0.grad_norm"][i_head]) > 1e-3 * b["s0.grad_norm"][i_head]
    assert abs(c["s0.grad_norm"][i_enc] - b["s0.grad_norm"][i_enc]) < 1e-4 * b["s0.grad_norm"][i_enc]


def test_abi_exports_head_mtl_ce():
    lib = L.load()
    for name in ("gdl_head_mtl_ce", "gdl_head_mtl_ce_workspace_bytes"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.gdl_head_mtl_ce.restype is ctypes.c_int and len(lib.gdl_head_mtl_ce.argtypes) == 25
    # a ticket counter on a line of its own + three loss terms per sample
    assert lib.gdl_head_mtl_ce_workspace_bytes(64) >= 4 + 3 * 64 * 4
    assert lib.gdl_head_mtl_ce_workspace_bytes(64) > lib.gdl_head_mtl_ce_workspace_bytes(4)
    nul = [None] * 4 + [1024, None, None, 0, None, 2.5, 1] + [None] * 9 + [4, 6, None, 0, None]
    assert lib.gdl_head_mtl_ce(*nul) != 0 and b"head_mtl_ce" in lib.gdl_last_error()
    one = ctypes.c_void_p(256)  # never dereferenced: the class count is refused on the host
    args = [one] * 4 + [1024, one, one, 0, one, 2.5, 1] + [one] * 9 + [4, 513, one, 1 << 20, None]
    assert lib.gdl_head_mtl_ce(*args) != 0 and b"512 classes" in lib.gdl_last_error()
    args[21], args[23] = 6, 8  # n_classes in range, a workspace that is too small
    assert lib.gdl_head_mtl_ce(*args) != 0 and b"workspace" in lib.gdl_last_error()


def test_switches_need_a_device_like_every_trainer():
    """No CPU path: the trainer refuses a CPU model whatever the switches say (the refusals that depend on them are GPU tests)."""
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier_DGL

    m = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=4))
    with pytest.raises(L.GdlError, match="cuda"):
        DGLTrainer(m, lr=1e-3, detach_fused=False, drop_head_uni=False)
