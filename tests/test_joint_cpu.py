"""CPU-only checks of the joint-training baselines (BASELINE config 1 for all four fusion heads): the mirror classes keep the
reference's names, parameter order and state layout (read off the fixtures tests/golden/make_golden_joint.py captured from
the imported reference), CPU tensors are refused, and the C ABI exports the joint heads' entry points."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from gdl import _lib as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = {"concat": "concat_cremad_b2", "sum": "joint_sum_tiny_b4", "gated": "joint_gated_tiny_b4", "film": "joint_film_tiny_b4"}
JOINT_SYMBOLS = ("gdl_head_gated_joint_fwd", "gdl_head_gated_joint_bwd", "gdl_head_film_joint_fwd", "gdl_head_film_joint_bwd")


def _args(fusion):
    return argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality="full", batch_size=4)


@pytest.mark.parametrize("fusion", ["concat", "sum", "gated", "film"])
def test_avclassifier_builds_with_the_reference_layout(fusion):
    from models import fusion_modules as fm
    from models.basic_model import AVClassifier

    m = AVClassifier(_args(fusion))
    cls = {"concat": fm.ConcatFusion, "sum": fm.SumFusion, "gated": fm.GatedFusion, "film": fm.FiLM}[fusion]
    assert type(m.fusion_module) is cls
    g = np.load(os.path.join(GOLD, FIXTURE[fusion] + ".npz"), allow_pickle=False)
    names = [str(n) for n in g["s0.grad_names"]]
    assert [n for n, _ in m.named_parameters()] == names  # the reference's names in its registration order
    bufs = [k[len("s0.buf."):] for k in g.files if k.startswith("s0.buf.")]
    assert set(m.state_dict().keys()) == set(names) | set(bufs)
    nh = {"concat": 2, "sum": 4, "gated": 6, "film": 4}[fusion]
    assert all(n.startswith("fusion_module.") for n in names[:nh]) and names[nh].startswith("audio_net.")
    if fusion == "gated":
        assert m.fusion_module.x_gate is True and m.fusion_module.fc_x.weight.shape == (512, 512)
    if fusion == "film":
        assert m.fusion_module.fc.weight.shape == (512, 512 * 512) and m.fusion_module.fc_out.weight.shape == (6, 512)
    # no CPU fallback: CPU tensors are refused loudly
    with pytest.raises(Exception):
        m(torch.zeros(1, 1, 65, 47), torch.zeros(1, 3, 2, 64, 64))


def test_unknown_fusion_method_and_film_width_are_refused():
    from models.basic_model import AVClassifier
    from models.fusion_modules import FiLM, GatedFusion, GatedFusion_DGL

    for method in ("film_like", "attention"):
        with pytest.raises(NotImplementedError):
            AVClassifier(_args(method))
    with pytest.raises(NotImplementedError):
        FiLM(output_dim=6)  # the reference's default dim=768 cannot take 512-wide features
    with pytest.raises(NotImplementedError):
        FiLM(input_dim=768, dim=512, output_dim=6)
    assert GatedFusion(output_dim=6, x_gate=False).x_gate is False
    with pytest.raises(NotImplementedError):
        GatedFusion_DGL(output_dim=6, x_gate=False)


def test_joint_heads_refuse_cpu_tensors():
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier
    from models.fusion_modules import GatedFusion, SumFusion

    x, y = torch.zeros(2, 512), torch.zeros(2, 512)
    for head in (SumFusion(output_dim=6), GatedFusion(output_dim=6), GatedFusion(output_dim=6, x_gate=False)):
        with pytest.raises(RuntimeError, match="GPU only"):
            head(x, y)
    with pytest.raises(L.GdlError):
        DGLTrainer(AVClassifier(_args("sum")), lr=1e-3, mode="joint")  # the model lives on the CPU


def test_joint_symbols_resolve():
    lib = L.load()
    for name in JOINT_SYMBOLS:
        assert name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(L.SIGNATURES[name][1])
    # argument checks run on the host before any launch: NULL pointers are reported the documented way
    assert lib.gdl_head_gated_joint_fwd(*([None] * 11), 1, 4, 6, None) != 0 and b"head_gated_joint_fwd" in lib.gdl_last_error()
    assert lib.gdl_head_film_joint_bwd(*([None] * 12), 4, 6, None, 0, None) != 0 and b"head_film_joint_bwd" in lib.gdl_last_error()


def test_joint_fixtures_record_the_float64_norm():
    """The step fixtures clip with the float64 norm of the float32 gradients and keep torch's own float32 value beside it
    (docs/parity_log.md: on the FiLM fixture the two differ by 1.1 %)."""
    for fusion, steps in (("sum", 2), ("gated", 2), ("film", 1)):
        g = np.load(os.path.join(GOLD, FIXTURE[fusion] + ".npz"), allow_pickle=False)
        cfg = json.loads(str(g["config"]))
        assert cfg["mode"] == "joint" and cfg["steps"] == steps and cfg["fusion"] == fusion
        for st in range(steps):
            gn = g[f"s{st}.grad_norm"]
            assert not g[f"s{st}.grad_is_none"].any()
            np.testing.assert_allclose(np.sqrt((gn ** 2).sum()), float(g[f"s{st}.total_norm"]), rtol=1e-12)
            np.testing.assert_allclose(float(g[f"s{st}.total_norm_torch32"]), float(g[f"s{st}.total_norm"]), rtol=2e-2)
