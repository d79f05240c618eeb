"""CPU-only checks of the drop-in boundary: the C-ABI library loads without a GPU and exports every
symbol include/gdl_hip.h declares, the ctypes binding covers all of them, the pure host queries
(table / workspace / tile counts, engine planning) behave, errors are reported the documented way,
and the Python mirror of the reference interface keeps the reference's names and ordering."""
import argparse
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))

from gdl import _lib as L  # noqa: E402

HEADER = os.path.join(ROOT, "include", "gdl_hip.h")


def header_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"GDL_API\s+[\w\s\*]+?\b(gdl_\w+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(L.SO_PATH)  # loads without a GPU: no HIP call happens at load time
    names = header_symbols()
    assert len(names) > 50
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in include/gdl_hip.h but not exported: {missing}"


def test_binding_table_matches_header():
    names = set(header_symbols())
    bound = set(L.SIGNATURES)
    assert names - bound == set(), f"no ctypes signature for {sorted(names - bound)}"
    assert bound - names == set(), f"bound but not declared in the header: {sorted(bound - names)}"


def test_host_queries_need_no_gpu():
    lib = L.load()
    bf16, f32 = L.dtype_code("bf16"), L.dtype_code("f32")
    # stem K padding: 147 -> 192 (bf16, 64-element K-steps), 49 -> 64
    # gather tables: 8 bytes per GEMM row; the permuted stride-2 data-gradient table carries row indices too
    N, H, W = 4, 56, 56
    assert lib.gdl_conv_table_bytes(L.GDL_GATHER_FWD if hasattr(L, "GDL_GATHER_FWD") else 0, N, H, W, 3, 3, 1, 1) == N * H * W * 8
    assert lib.gdl_conv_table_bytes(0, N, H, W, 3, 3, 2, 1) == N * 28 * 28 * 8
    assert lib.gdl_conv_table_bytes(1, N, H, W, 3, 3, 1, 1) == N * H * W * 8
    assert lib.gdl_conv_table_bytes(1, N, H, W, 3, 3, 2, 1) > N * H * W * 12
    # BatchNorm partial rows of a convolution = its M-tiles; workspace queries are monotone in the problem size
    t_small = lib.gdl_conv_bn_tiles(bf16, 2, 56, 56, 64, 64, 3, 3, 1, 1)
    t_big = lib.gdl_conv_bn_tiles(bf16, 192, 56, 56, 64, 64, 3, 3, 1, 1)
    assert 0 < t_small < t_big
    w_small = lib.gdl_conv_wgrad_workspace_bytes(bf16, 2, 56, 56, 64, 64, 3, 3, 1, 1)
    w_big = lib.gdl_conv_wgrad_workspace_bytes(bf16, 192, 56, 56, 64, 64, 3, 3, 1, 1)
    assert 0 < w_small <= w_big
    assert lib.gdl_bn_bwd_blocks(1 << 20, 64) <= 2048 and lib.gdl_bn_bwd_blocks(1024, 64) >= 1


def test_slab_planner_at_the_benchmark_shapes():
    """Which kernel the >= 128-channel 3x3 stride-1 layers of the B = 64 CREMA-D step run on, read off
    the BatchNorm partial-row counts the C ABI reports -- forward and data gradient must agree (the engine sizes one buffer for
    both): the persistent slab kernel writes one row per BLOCK (its grid: at most 512, eight equal XCD shares), the round-5 kernel
    one per M-tile.  f32 (the exact-parity mode) never uses the persistent kernel.  No GPU needed: the planner is host code."""
    lib = L.load()
    bf16, f32 = L.dtype_code("bf16"), L.dtype_code("f32")
    want = {  # (images, channels, H, W): rows
        (192, 128, 28, 28): 512,  # visual layer 2: 784 tiles of 192 rows on 512 persistent blocks
        (192, 256, 14, 14): 392,  # visual layer 3: 196 M-tiles x 2 N-tiles, one tile per block
        (192, 512, 7, 7): 200,    # visual layer 4: 49 x 4 = 196 items -> 8 x 25 blocks
        (64, 128, 33, 24): 396,   # audio layer 2: the round-5 kernel (128-row tiles, two slab buffers): its M-tiles
        (64, 256, 17, 12): 136,   # audio layer 3: 68 x 2
        (64, 512, 9, 6): 112,     # audio layer 4: 128-row tiles, 27 x 4 = 108 items -> 8 x 14 blocks
    }
    for (N, C, H, W), rows in want.items():
        assert lib.gdl_conv_bn_tiles(bf16, N, H, W, C, C, 3, 3, 1, 1) == rows, (N, C, H, W)
        assert lib.gdl_conv_dgrad_bn_tiles(bf16, N, H, W, C, C, 3, 3, 1, 1) == rows, (N, C, H, W)
        assert lib.gdl_conv_bn_tiles(f32, N, H, W, C, C, 3, 3, 1, 1) == -(-N * H * W // 128), (N, C, H, W)
    # 128 -> 384 channels (three N-tiles): 786 items on 512 persistent blocks would change a block's N-tile between its items,
    # so the shape keeps the 192-row tiles of the round-5 kernel -- 262 M-tiles
    assert lib.gdl_conv_bn_tiles(bf16, 64, 28, 28, 128, 384, 3, 3, 1, 1) == 262


def test_engine_plans_without_gpu_and_reports_errors():
    lib = L.load()
    h = ctypes.c_void_p()
    L.call("gdl_encoder_create", ctypes.byref(h), L.GDL_VISUAL, L.dtype_code("bf16"), 2, 3, 224, 224)
    try:
        ws = lib.gdl_encoder_workspace_bytes(h)
        assert ws > 0
        numel = (ctypes.c_int64 * L.ENC_NPARAMS)()
        L.call("gdl_encoder_param_numel", h, numel)
        assert sum(numel) == 11176512  # visual ResNet18 without fc (SURVEY: 11.18 M)
        n, hh, ww = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        L.call("gdl_encoder_out_shape", h, ctypes.byref(n), ctypes.byref(hh), ctypes.byref(ww))
        assert (n.value, hh.value, ww.value) == (6, 7, 7)
        # backward without a training forward: documented state error, message available
        grads = (ctypes.c_void_p * L.ENC_NPARAMS)()
        rc = lib.gdl_encoder_backward(h, None, None, grads, None)
        assert rc != 0 and lib.gdl_last_error()
    finally:
        lib.gdl_encoder_destroy(h)
    h2 = ctypes.c_void_p()
    with pytest.raises(L.GdlError):
        L.call("gdl_encoder_create", ctypes.byref(h2), L.GDL_AUDIO, L.dtype_code("bf16"), 2, 3, 257, 188)  # audio takes T=1
    big = ctypes.c_void_p()
    L.call("gdl_encoder_create", ctypes.byref(big), L.GDL_VISUAL, L.dtype_code("bf16"), 64, 3, 224, 224)
    small_ws = ws
    try:
        assert lib.gdl_encoder_workspace_bytes(big) > 12 * small_ws  # sized for the real batch (32x the samples; tables and fold rows are fixed)
    finally:
        lib.gdl_encoder_destroy(big)


def test_mirror_keeps_reference_interface():
    from models.basic_model import AVClassifier, AVClassifier_DGL
    from models.fusion_modules import ConcatFusion, ConcatFusion_DGL
    from utils.utils import setup_seed, weight_init

    setup_seed(0)
    args = argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full")
    m = AVClassifier_DGL(args)
    m.apply(weight_init)
    names = [n for n, _ in m.named_parameters()]
    # main_dgl.py:117-121 drops the gradients of parameters whose name contains "fusion"; registration order
    # fusion (4) -> audio_net (60) -> visual_net (60) as in basic_model.py:11-61
    assert names[:4] == ["fusion_module.fc_out.weight", "fusion_module.fc_out.bias", "fusion_module.fc_auxi.weight",
                         "fusion_module.fc_auxi.bias"]
    assert names[4].startswith("audio_net.") and names[64].startswith("visual_net.") and len(names) == 124
    assert m.audio_net.conv1.weight.shape == (64, 1, 7, 7) and m.visual_net.conv1.weight.shape == (64, 3, 7, 7)
    assert m.fusion_module.fc_out.weight.shape == (6, 1024)
    sd = m.state_dict()
    assert "audio_net.bn1.num_batches_tracked" in sd and "visual_net.layer4.1.bn2.running_var" in sd
    assert isinstance(m.fusion_module, ConcatFusion_DGL) and isinstance(AVClassifier(args).fusion_module, ConcatFusion)
    from models.fusion_modules import SumFusion_DGL

    ms = AVClassifier_DGL(argparse.Namespace(fusion_method="sum", dataset="KineticSound", modality="full"))
    assert isinstance(ms.fusion_module, SumFusion_DGL)
    assert [n for n, _ in ms.named_parameters()][:4] == ["fusion_module.fc_x.weight", "fusion_module.fc_x.bias",
                                                         "fusion_module.fc_y.weight", "fusion_module.fc_y.bias"]
    assert ms.fusion_module.fc_x.weight.shape == (34, 512)
    mg = AVClassifier_DGL(argparse.Namespace(fusion_method="gated", dataset="CREMAD", modality="full"))
    assert [n for n, _ in mg.named_parameters()][:6] == ["fusion_module.fc_x.weight", "fusion_module.fc_x.bias",
                                                         "fusion_module.fc_y.weight", "fusion_module.fc_y.bias",
                                                         "fusion_module.fc_out.weight", "fusion_module.fc_out.bias"]
    assert mg.fusion_module.fc_out.weight.shape == (6, 512) and mg.fusion_module.x_gate is True
    for method in ("film_like", "attention"):
        with pytest.raises(NotImplementedError):
            AVClassifier_DGL(argparse.Namespace(fusion_method=method, dataset="CREMAD", modality="full"))
    # no CPU fallback: CPU tensors are refused loudly
    with pytest.raises(Exception):
        m(torch.zeros(1, 1, 257, 188), torch.zeros(1, 3, 3, 224, 224))


def test_seeded_init_matches_reference():
    """setup_seed(0) + AVClassifier_DGL(args) + apply(weight_init) gives the reference's initial weights (golden
    captured from the imported reference: per-tensor sum and sum of magnitudes), for every head this build provides."""
    import numpy as np

    from models.basic_model import AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    g = np.load(os.path.join(ROOT, "tests", "golden", "seeded_init.npz"))
    for fusion in ("concat", "sum", "gated", "film"):
        setup_seed(0)
        m = AVClassifier_DGL(argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality="full", batch_size=2))
        m.apply(weight_init)
        sd = m.state_dict()
        assert list(sd.keys()) == [str(k) for k in g[fusion + ".keys"]]
        got = np.stack([[v.double().sum().item(), v.double().abs().sum().item()] for v in sd.values()])
        np.testing.assert_allclose(got, g[fusion + ".sums"], rtol=1e-12, atol=1e-12)


# What the reference training script (main_dgl.py) imports from the package at module level -- every name must resolve to
# the mirror or the synthetic dataset stand-ins -- and the tensorboard writer it imports before them.
REFERENCE_SCRIPT_IMPORTS = {
    "torch.utils.tensorboard": ["SummaryWriter"],
    "dataset.CramedDataset": ["CramedDataset", "CramedDataset_swin"],
    "dataset.KSDataset": ["KSDataset"],
    "dataset.VGGSoundDataset": ["VGGSound"],
    "dataset.AVEDataset": ["AVEDataset"],
    "models.basic_model": ["AVClassifier_DGL"],
    "utils.utils": ["setup_seed", "weight_init"],
    "dataset.Kinect400": ["Kinect400"],
}


def test_reference_script_starts_on_the_dropin_modules(tmp_path):
    """A training script written against the reference's modules starts on the mirror (SURVEY 8(b) "Who calls"):
    gdl.run_reference puts the package first on sys.path -- models.basic_model / utils.utils / dataset.* resolve to the
    mirror and the synthetic dataset stand-ins -- and supplies a no-op SummaryWriter when the tensorboard package is
    absent.  The script here is a stand-in for the reference's main_dgl.py: its module-level imports of the package
    (REFERENCE_SCRIPT_IMPORTS), then argument parsing -- the phase of main_dgl.py that runs without a GPU."""
    import subprocess
    import sys

    script = tmp_path / "main_dgl.py"
    script.write_text(
        "import argparse\nimport importlib\nimport os\n"
        f"for mod, names in {REFERENCE_SCRIPT_IMPORTS!r}.items():\n"
        "    m = importlib.import_module(mod)\n"
        "    for n in names:\n"
        "        getattr(m, n)\n"
        "    if not mod.startswith('torch.'):\n"
        "        print('resolved', mod, os.path.abspath(m.__file__))\n"
        "ap = argparse.ArgumentParser()\n"
        "ap.add_argument('--fusion_method', default='concat', choices=['sum', 'concat', 'gated', 'film'])\n"
        "ap.add_argument('--alpha', default=4.0, type=float)\n"
        "ap.parse_args()\n")
    pkg = os.path.join(ROOT, "iccv2025-gdl_amd")
    r = subprocess.run([sys.executable, "-m", "gdl.run_reference", str(script), "--help"], cwd=pkg, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--fusion_method" in r.stdout and "--alpha" in r.stdout
    resolved = [ln.split()[2] for ln in r.stdout.splitlines() if ln.startswith("resolved ")]
    assert len(resolved) == len(REFERENCE_SCRIPT_IMPORTS) - 1 and all(f.startswith(pkg + os.sep) for f in resolved), r.stdout
    probe = ("import sys; sys.path.insert(0, %r); import dataset.CramedDataset as d, models.basic_model as m, utils.utils as u;"
             "from dataset.KSDataset import KSDataset; ds = KSDataset(None, mode='test'); s, i, l = ds[0];"
             "assert tuple(s.shape) == (129, 626) and tuple(i.shape) == (3, 3, 224, 224) and 0 <= l < 34;"
             "print(d.__file__, m.__file__, u.__file__)") % pkg
    r = subprocess.run([sys.executable, "-c", probe], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count(pkg) == 3


def test_swin_mirror_matches_reference_layout():
    """The Swin mirror registers the reference's parameters in the reference's order (the order fx.swin_param_shapes
    restates; tests/golden/make_golden.py asserted it against the imported SwinTransformer when the goldens were made) and
    offers the reference's buffers; unsupported constructor arguments are refused rather than ignored."""
    import argparse

    import pytest
    from models.basic_model import AVClassifier_DGL_Swin
    from models.swin_transformer import SwinTransformer

    from oracle import fixtures as fx

    args = argparse.Namespace(pe=0)
    for cfg in (fx.SWIN_T, fx.SWIN_TINY2):
        net = SwinTransformer(args, "visual", img_size=cfg["img"], patch_size=cfg["patch"], embed_dim=cfg["embed"],
                              depths=list(cfg["depths"]), num_heads=list(cfg["heads"]), window_size=cfg["window"],
                              mlp_ratio=float(cfg["mlp"]), drop_path_rate=0.)
        want = fx.swin_param_shapes(cfg)
        assert [(n, tuple(p.shape)) for n, p in net.named_parameters()] == [(n, tuple(s)) for n, s in want.items()]
        bufs = dict(net.named_buffers())
        assert "layers.0.blocks.0.attn.relative_position_index" in bufs and "layers.0.blocks.1.attn_mask" in bufs
        assert "layers.0.blocks.0.attn_mask" not in bufs  # un-shifted blocks have none (a None buffer is not in the state)
        assert net.num_features == cfg["embed"] << (len(cfg["depths"]) - 1)
    # the reference's default drop_path_rate = 0.1 (swin_transformer.py:516): constructible, and no mode is refused any more
    # (round 4: a training forward draws the DropPath masks); a CPU tensor is -- there is no CPU path
    dflt = SwinTransformer(args, "visual", embed_dim=96, depths=[2, 2], num_heads=[3, 6])
    assert dflt.drop_path_rate == pytest.approx(0.1)
    dflt.train()
    with pytest.raises(RuntimeError, match="GPU only"):
        dflt(torch.zeros(1, 3, 1, 224, 224))
    # the masks: drawn like the reference's blocks draw them (same generator, same order: attention branch then Mlp branch, block
    # by block; probability linspace(0, rate, blocks); the first block is nn.Identity and draws nothing)
    from models.swin_transformer import drop_path_scales
    from oracle import swin_oracle as so

    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    sc = drop_path_scales(fx.SWIN_T, 0.4, 64, "cpu", generator=g1)
    assert tuple(sc.shape) == (12, 2, 64) and bool((sc[0] == 1).all()) and torch.equal(sc, so.drop_path_scales(fx.SWIN_T, 0.4, 64, generator=g2))
    keep = 1.0 - torch.linspace(0, 0.4, 12)
    for k in range(1, 12):
        vals = set(sc[k].reshape(-1).tolist())
        assert vals <= {0.0, float(torch.tensor(1.0) / keep[k])} and (k < 6 or 0.0 in vals)
    with pytest.raises(NotImplementedError):
        SwinTransformer(argparse.Namespace(pe=1), "visual", drop_path_rate=0.)
    m = AVClassifier_DGL_Swin(argparse.Namespace(fusion_method="concat", dataset="VGGSound", modality="full", pe=0))
    P, _ = fx.swin_dgl_state(309, fx.SWIN_T)
    assert [n for n, _ in m.named_parameters()] == list(P)
    assert m.fusion_module.fc_out.weight.shape == (309, 512 + 768)


def test_isa_screen_no_cross_half_packed_add():
    """tools/check_isa.sh on the in-tree build: no object of libgdl_hip.so may contain `v_pk_add_f32 .. op_sel:[0,1] op_sel_hi:[1,0]`,
    the packed-f32 form the SLP vectoriser makes of the epilogues' statistics and that gives run-to-run different BatchNorm sums on
    MI355X (csrc/Makefile; the GPU side is tests/test_ops_gpu.py::test_bn_sums_determinism_full_size)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = os.path.join(root, "iccv2025-gdl_amd", "csrc", "build")
    if not any(f.endswith(".o") for f in os.listdir(build)):
        pytest.skip("objects not kept next to the library")
    r = subprocess.run(["bash", os.path.join(root, "tools", "check_isa.sh"), build], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "check_isa: 0 cross-half" in r.stdout
