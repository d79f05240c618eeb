"""CPU-only checks of the unimodal baselines (the audio encoder alone / the visual encoder alone with a Linear(512, n)
classifier): the mirror's two modes keep the reference's names, registration order and state layout (read off the fixtures
tests/golden/make_golden_unimodal.py captured from the imported reference), the C ABI exports the classifier's entry points,
and everything that would need a CPU path is refused."""
import argparse
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from gdl import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLS_SYMBOLS = ("gdl_head_cls_fwd", "gdl_head_cls_bwd", "gdl_head_cls_ce")


def _args(modality, fusion="concat"):
    return argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality=modality, batch_size=4)


@pytest.mark.parametrize("modality", ["audio", "visual"])
def test_mirror_builds_the_unimodal_modes_with_the_reference_layout(modality):
    from models.basic_model import AVClassifier_DGL
    from models.fusion_modules import ConcatFusion_DGL

    other = "visual" if modality == "audio" else "audio"
    m = AVClassifier_DGL(_args(modality))
    g = np.load(os.path.join(GOLD, f"uni_{modality}_tiny_b4.npz"), allow_pickle=False)
    cfg = json.loads(str(g["config"]))
    assert cfg["mode"] == "unimodal" and cfg["modality"] == modality
    names = [str(n) for n in g["param_names"]]
    assert [n for n, _ in m.named_parameters()] == names  # the reference's names in its registration order
    assert names[:4] == ["fusion_module.fc_out.weight", "fusion_module.fc_out.bias", "fusion_module.fc_auxi.weight",
                         "fusion_module.fc_auxi.bias"]
    assert all(n.startswith(modality + "_net.") for n in names[4:64]) and len(names) == 66
    assert names[64:] == [modality + "_classifier.weight", modality + "_classifier.bias"]
    assert isinstance(m.fusion_module, ConcatFusion_DGL)  # constructed, unused: reference checkpoints load strictly
    cls = getattr(m, modality + "_classifier")
    assert isinstance(cls, torch.nn.Linear) and cls.weight.shape == (6, 512) and cls.bias.shape == (6,)
    assert not hasattr(m, other + "_net") and not hasattr(m, other + "_classifier")
    assert m.modality == modality
    # the fixture's state (every parameter and buffer the reference's state_dict has) loads strictly
    bufs = [k[len("s0.buf."):] for k in g.files if k.startswith("s0.buf.")]
    assert set(m.state_dict().keys()) == set(names) | set(bufs)
    sd = {k: torch.zeros_like(v) for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    # the fusion tensors get no gradient in the reference; the fixture says so
    none = g["s0.grad_is_none"]
    assert [n for n, f in zip(names, none) if f] == names[:4]


def test_other_modalities_keep_raising():
    from models.basic_model import AVClassifier_DGL

    for modality in ("both", "text", None):
        with pytest.raises(NotImplementedError):
            AVClassifier_DGL(_args(modality))
    with pytest.raises(NotImplementedError):
        AVClassifier_DGL(_args("audio", fusion="attention"))
    assert AVClassifier_DGL(_args("full")).modality == "full"


def test_header_exports_the_classifier_entry_points():
    src = open(os.path.join(ROOT, "include", "gdl_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"GDL_API\s+[\w\s\*]+?\b(gdl_\w+)\s*\(", src))
    lib = L.load()
    for name in CLS_SYMBOLS:
        assert name in declared and name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(L.SIGNATURES[name][1])
    # argument checks run on the host before any launch: NULL pointers and a width other than 512 are reported
    assert lib.gdl_head_cls_fwd(None, None, None, None, 4, 6, 512, None) != 0 and b"head_cls_fwd" in lib.gdl_last_error()
    assert lib.gdl_head_cls_bwd(None, None, None, None, None, None, 4, 6, 512, None) != 0 and b"head_cls_bwd" in lib.gdl_last_error()
    assert lib.gdl_head_cls_ce(None, None, None, None, 1.0, None, None, None, None, 4, 6, 512, None) != 0
    assert b"head_cls_ce" in lib.gdl_last_error()
    one = ctypes.c_void_p(256)  # never dereferenced: the width is refused on the host
    assert lib.gdl_head_cls_fwd(one, one, one, one, 4, 6, 768, None) != 0 and b"width" in lib.gdl_last_error()


def test_refusals():
    import gdl
    from gdl.unimodal import UnimodalTrainer
    from models.basic_model import AVClassifier_DGL, Classifier

    assert gdl.UnimodalTrainer is UnimodalTrainer
    audio = AVClassifier_DGL(_args("audio"))
    with pytest.raises(L.GdlError, match="cuda"):
        UnimodalTrainer(audio, lr=1e-3)  # the model lives on the CPU
    with pytest.raises(L.GdlError, match="DGLTrainer"):
        UnimodalTrainer(AVClassifier_DGL(_args("full")), lr=1e-3)
    allocs = []
    real = torch.empty
    try:
        torch.empty = lambda *a, **k: (allocs.append(a), real(*a, **k))[1]
        with pytest.raises(ValueError, match="optimizer"):
            UnimodalTrainer(audio, lr=1e-3, optimizer="rmsprop")
    finally:
        torch.empty = real
    assert not allocs  # refused before anything is allocated
    with pytest.raises(L.GdlError, match="process_group"):
        UnimodalTrainer(audio, lr=1e-3, process_group=object())
    # no CPU fallback: CPU tensors are refused loudly by the modes' forward and by the classifier itself
    with pytest.raises(RuntimeError, match="GPU only"):
        audio(torch.zeros(4, 1, 65, 47), None)
    with pytest.raises(RuntimeError, match="GPU only"):
        AVClassifier_DGL(_args("visual"))(None, torch.zeros(4, 3, 2, 64, 64))
    with pytest.raises(RuntimeError, match="GPU only"):
        Classifier(512, 6)(torch.zeros(2, 512))
