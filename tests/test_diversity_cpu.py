"""CPU-only checks of the feature-diversity monitor: the project's float64 statement (tests/diversity_ref.py) against the
values the reference's own function gave (tests/golden/make_golden_diversity.py), its closed forms, the refusals of the C ABI
that need no device, and the trainers' argument checks."""
import argparse
import ctypes
import inspect
import os

import numpy as np
import pytest

import diversity_ref as dr
from gdl import _lib as L

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diversity_ref.npz"), allow_pickle=False)
SEED = 7  # make_golden_diversity.SEED
OP_CASES = [(k, s) for k in ("relu", "shift32") for s in dr.SHAPES] + [("same", dr.SAME_SHAPE), ("zero_row", (3, 7, 7))]


@pytest.mark.parametrize("kind,shape", OP_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_ref_against_the_reference_function(kind, shape):
    """diversity_ref agrees with the reference function's float64 run to 1e-12 (NaN where it gives NaN), and that function's
    float32 run stays within 2.2e-6 of its float64 run: the room the GPU test's 1e-4 leaves is the kernel's own."""
    n, h, w = shape
    pre = f"op.{kind}.{n}x{h}x{w}."
    d, m = dr.diversity_ref(dr.make_map(SEED, n, h, w, kind))
    np.testing.assert_allclose(d, GOLD[pre + "d64"], rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(m, GOLD[pre + "m64"], rtol=1e-12, atol=0, equal_nan=True)
    ok = np.isfinite(GOLD[pre + "d64"])
    np.testing.assert_allclose(GOLD[pre + "d32"][ok], GOLD[pre + "d64"][ok], rtol=2.2e-6, atol=0)


def test_closed_forms():
    """P = 1: R = [C - 1], d = 511 exactly.  All positions equal: every R_pq = C - 1, ||R||_F = P (C - 1), d = 511 / P.
    One all-zero position: NaN for that image alone, NaN mean."""
    d, m = dr.diversity_ref(dr.make_map(3, 4, 1, 1, "relu"))
    np.testing.assert_allclose(d, 511.0, rtol=1e-13)
    for h, w in ((2, 2), (7, 7), (5, 20)):
        d, m = dr.diversity_ref(dr.make_map(3, 2, h, w, "same"))
        np.testing.assert_allclose(d, 511.0 / (h * w), rtol=1e-12)
    x = dr.make_map(3, 3, 7, 7, "zero_row")
    i, p = dr.zero_row_index(3, 7, 7)
    assert not x.reshape(3, 512, 49)[i, :, p].any()
    d, m = dr.diversity_ref(x)
    assert np.isnan(d[i]) and np.isfinite(np.delete(d, i)).all() and np.isnan(m)


def test_fold_mean_is_the_mean():
    r = np.random.default_rng(5)
    for n in (1, 3, 64, 256, 257, 300, 1000):
        v = (r.random(n) * 60 + 1).astype(np.float32)
        assert abs(float(dr.fold_mean(v)) - v.astype(np.float64).mean()) <= 1e-6 * v.astype(np.float64).mean()


def test_step_fixture_is_consistent():
    """the step fixture: both encoders' maps of the tiny batch ([4, 512, 3, 2] audio, [8, 512, 2, 2] visual), float32 within
    2.2e-6 of float64"""
    assert tuple(GOLD["step.a.shape"]) == (4, 512, 3, 2) and tuple(GOLD["step.v.shape"]) == (8, 512, 2, 2)
    for k in ("a", "v"):
        np.testing.assert_allclose(GOLD[f"step.{k}.d32"], GOLD[f"step.{k}.d64"], rtol=2.2e-6)
        np.testing.assert_allclose(GOLD[f"step.{k}.m64"], GOLD[f"step.{k}.d64"].mean(), rtol=1e-12)


def test_abi_refusals_need_no_gpu():
    lib = L.load()
    for name in ("gdl_feature_diversity", "gdl_feature_diversity_workspace_bytes", "gdl_encoder_feature_diversity"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert len(lib.gdl_feature_diversity.argtypes) == 12 and len(lib.gdl_encoder_feature_diversity.argtypes) == 7
    wsb = lib.gdl_feature_diversity_workspace_bytes
    assert wsb(64) == 256 + 64 * 4 and wsb(300) == 256 + 300 * 4  # the counter on its own 256-byte line + n_img floats
    one = ctypes.c_void_p(256)  # never dereferenced: every case below is refused on the host
    f32, bf16, nhwc, nchw = L.GDL_F32, L.GDL_BF16, L.GDL_LAYOUT_NHWC, L.GDL_LAYOUT_NCHW

    def refused(match, map_=one, dtype=f32, layout=nhwc, n=2, P=49, C=512, mean=one, ws=one, ws_bytes=1 << 20):
        rc = lib.gdl_feature_diversity(map_, dtype, layout, n, P, C, None, mean, None, ws, ws_bytes, None)
        assert rc != 0 and match in lib.gdl_last_error(), (rc, lib.gdl_last_error())

    refused(b"C = 512", C=256)
    refused(b"[1, 256]", P=0)
    refused(b"[1, 256]", P=257)
    refused(b"n_img", n=0)
    refused(b"null", map_=None)
    refused(b"null", mean=None)
    refused(b"null", ws=None)
    refused(b"workspace", ws_bytes=256 + 2 * 4 - 1)
    refused(b"NCHW", dtype=bf16, layout=nchw)
    refused(b"layout", layout=2)
    refused(b"aligned", map_=ctypes.c_void_p(260))
    refused(b"256-byte aligned", ws=ctypes.c_void_p(260))  # the counter's line must hold nothing else


def test_engine_refuses_before_any_forward():
    lib = L.load()
    h = ctypes.c_void_p()
    L.call("gdl_encoder_create", ctypes.byref(h), L.GDL_AUDIO, L.dtype_code("f32"), 2, 1, 65, 47)
    try:
        one = ctypes.c_void_p(256)
        rc = lib.gdl_encoder_feature_diversity(h, None, one, None, one, 1 << 20, None)
        assert rc != 0 and b"no forward" in lib.gdl_last_error()
        rc = lib.gdl_encoder_feature_diversity(h, None, None, None, one, 1 << 20, None)
        assert rc != 0 and b"null" in lib.gdl_last_error()
    finally:
        lib.gdl_encoder_destroy(h)


def test_python_surface_without_a_device():
    """gdl.feature_diversity has no CPU path; the trainers take `diversity` (off by default) and still refuse a CPU model."""
    import torch

    import gdl
    from gdl.trainer import DGLTrainer
    from gdl.unimodal import UnimodalTrainer
    from models.basic_model import AVClassifier_DGL

    with pytest.raises(L.GdlError, match="no CPU path"):
        gdl.feature_diversity(torch.zeros(1, 512, 2, 2))
    for cls in (DGLTrainer, UnimodalTrainer):
        assert inspect.signature(cls.__init__).parameters["diversity"].default is False
        assert callable(cls.epoch_diversity)
    m = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=4))
    with pytest.raises(L.GdlError, match="cuda"):
        DGLTrainer(m, lr=1e-3, diversity=True)
    ma = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="audio", batch_size=4))
    with pytest.raises(L.GdlError, match="cuda"):
        UnimodalTrainer(ma, lr=1e-3, diversity=True)
