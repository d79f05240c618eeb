"""gdl_frames_resized_crop / gdl.data.resized_crop_frames / augment_frames on the GPU: crop, Pillow's antialiased bilinear resize,
flip, ToTensor and Normalize in one launch, held bit for bit to the NumPy restatement tests/resize_ref.py (which
tests/test_augment_cpu.py pins to torch's CPU resize).  Bit-identical is a fair demand: everything on pixels is integer
arithmetic and the normalise is the expression test_normalize_frames already holds to assert_array_equal."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resize_ref as rr  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gdl import data as gd  # noqa: E402
from gpu_util import DEV  # noqa: E402

MEAN, STD = gd.IMAGENET_MEAN, gd.IMAGENET_STD


def _call_abi(imgs, boxes, flips, B, T, out_h, out_w, mean=MEAN, std=STD, n_img=None, edit=None):
    """Pack the frames as the header describes and call the C entry point directly; returns the device output.  edit(rows)
    may change the descriptor rows before they go to the device."""
    rows, chunks, off = [], [], 0
    for img, box, flip in zip(imgs, boxes, flips):
        h, w = img.shape[:2]
        t, l, bh, bw = (0, 0, h, w) if box is None else box
        rows.append([off, h, w, t, l, bh, bw, int(flip)])
        pad = (-img.size) % 4
        chunks.append(np.concatenate([img.reshape(-1), np.zeros(pad, np.uint8)]))
        off += img.size + pad
    if edit is not None:
        edit(rows)
    src = torch.from_numpy(np.concatenate(chunks)).to(DEV)
    desc = torch.tensor(rows, dtype=torch.int64).to(DEV)
    out = torch.full((B, 3, T, out_h, out_w), 7.0, dtype=torch.float32, device=DEV)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    L.call("gdl_frames_resized_crop", L.ptr(src), src.numel(), L.ptr(desc), len(imgs) if n_img is None else n_img, B, T, out_h,
           out_w, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), L.ptr(out), L.cur_stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("i", range(len(rr.CASES)), ids=[c[0] for c in rr.CASES])
def test_abi_bit_identical_cases(i):
    """Every case of the CPU test, flipped and not flipped in one launch (T = 1: plain [n_img][3][h][w])."""
    case = rr.CASES[i]
    _, _, _, box, oh, ow = case
    img = rr.case_image(i, case)
    got = _call_abi([img, img], [box, box], [False, True], 2, 1, oh, ow).cpu().numpy()
    assert got.shape == (2, 3, 1, oh, ow)
    for n, flip in enumerate((False, True)):
        np.testing.assert_array_equal(got[n, :, 0], rr.augment(img, box, flip, (oh, ow), MEAN, STD))


def test_abi_mixed_sizes_flips_and_permuted_store():
    """B = 4, T = 3: twelve frames of three source sizes (one with an odd byte count, so later frames start at padded offsets and
    rows start at every byte alignment), boxes and flips mixed, other mean / std; the [B][3][T][h][w] store checked element for
    element.  Then T = 1 on the same frames."""
    rng = np.random.default_rng(21)
    shapes = [(90, 121), (360, 480), (233, 77)]
    imgs, boxes, flips = [], [], []
    for n in range(12):
        H, W = shapes[n % 3]
        imgs.append(rr.noise_image(50 + n, H, W))
        bh, bw = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        boxes.append(None if n == 4 else (int(rng.integers(0, H - bh + 1)), int(rng.integers(0, W - bw + 1)), bh, bw))
        flips.append(bool(n % 2) ^ (n > 6))
    mean, std = (0.1, 0.5, 0.9), (0.3, 1.0, 0.7)
    for (B, T), size in (((4, 3), (224, 224)), ((12, 1), (56, 72))):
        got = _call_abi(imgs, boxes, flips, B, T, size[0], size[1], mean, std).cpu().numpy()
        for n in range(12):
            want = rr.augment(imgs[n], boxes[n], flips[n], size, mean, std)
            np.testing.assert_array_equal(got[n // T, :, n % T], want, err_msg=f"image {n}, B {B}, T {T}")


def test_whole_224_frames_reduce_to_normalize_frames():
    """boxes=None on 224 x 224 frames, no flip: both passes are the identity, so the new entry point gives gd.normalize_frames'
    output bit for bit (in the trainer's layout: [B, T, 3, H, W] -> [B, 3, T, H, W])."""
    u8 = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (4, 3, 224, 224, 3), dtype=np.uint8)).to(DEV)
    got = gd.resized_crop_frames(u8, T=3)
    want = gd.normalize_frames(u8).permute(0, 2, 1, 3, 4)
    assert tuple(got.shape) == (4, 3, 3, 224, 224) and got.is_contiguous()
    assert torch.equal(got, want)


def test_augment_frames_eval_and_train():
    """augment_frames(train=False) is Resize((224, 224)) as restated; augment_frames(train=True) with a fixed generator equals the
    restatement on the boxes and flips the same generator yields on the host.  Frames as one tensor and as a list of sizes."""
    shapes = [(120, 160), (97, 131), (240, 200), (120, 160)]
    imgs = [rr.noise_image(70 + n, *shapes[n]) for n in range(4)]
    frames = [torch.from_numpy(a).to(DEV) for a in imgs]
    got = gd.augment_frames(frames, 2, False).cpu().numpy()
    assert got.shape == (2, 3, 2, 224, 224)
    for n in range(4):
        np.testing.assert_array_equal(got[n // 2, :, n % 2], rr.augment(imgs[n], None, False, 224, MEAN, STD))
    got = gd.augment_frames(frames, 2, True, generator=torch.Generator().manual_seed(11)).cpu().numpy()
    boxes, flips = gd.random_augment_params(shapes, generator=torch.Generator().manual_seed(11))
    assert len({tuple(b) for b in boxes.tolist()}) == 4
    for n in range(4):
        want = rr.augment(imgs[n], tuple(boxes[n].tolist()), bool(flips[n]), 224, MEAN, STD)
        np.testing.assert_array_equal(got[n // 2, :, n % 2], want)
    same = np.stack([rr.noise_image(90 + n, 64, 80) for n in range(6)]).reshape(2, 3, 64, 80, 3)
    got = gd.augment_frames(torch.from_numpy(same).to(DEV), 3, True, generator=torch.Generator().manual_seed(5), size=(48, 40))
    boxes, flips = gd.random_augment_params([(64, 80)] * 6, generator=torch.Generator().manual_seed(5))
    assert tuple(got.shape) == (2, 3, 3, 48, 40)
    for n in range(6):
        want = rr.augment(same.reshape(6, 64, 80, 3)[n], tuple(boxes[n].tolist()), bool(flips[n]), (48, 40), MEAN, STD)
        np.testing.assert_array_equal(got[n // 3, :, n % 3].cpu().numpy(), want)


def test_full_size_batch_feeds_a_step():
    """B = 64, T = 3, 360 x 480 sources, seeded boxes and flips: the grid at its real size, eight images compared, and the result
    is the `image` of one DGLTrainer.step, which must finish with finite losses."""
    from gdl.trainer import DGLTrainer
    from test_step_gpu import _FULL_CFG, _batch, _make_model

    B, T = 64, 3
    u8 = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (B * T, 360, 480, 3), dtype=np.uint8))
    g = torch.Generator().manual_seed(2)
    boxes = gd.random_resized_crop_params([(360, 480)] * (B * T), generator=g)
    flips = gd.random_flips(B * T, generator=g)
    image = gd.resized_crop_frames(u8.to(DEV), boxes, flips, T=T)
    assert tuple(image.shape) == (B, 3, T, 224, 224)
    assert bool(torch.isfinite(image).all())
    for n in (0, 1, 2, 50, 95, 96, 190, 191):
        want = rr.augment(u8[n].numpy(), tuple(boxes[n].tolist()), bool(flips[n]), 224, MEAN, STD)
        np.testing.assert_array_equal(image[n // T, :, n % T].cpu().numpy(), want, err_msg=f"image {n}")
    cfg = dict(_FULL_CFG["cremad"])
    model = _make_model(cfg, "bf16")
    model.train()
    tr = DGLTrainer(model, lr=2e-3, alpha=cfg["alpha"], mode="dgl")
    spec, _, label = _batch(cfg, 0)
    tr.step(spec, image, label)
    r = tr.read()
    for k in ("loss_f", "loss_a", "loss_v", "total_norm"):
        assert np.isfinite(r[k]), (k, r[k])


def test_unaligned_views_and_lists_are_packed():
    """A contiguous view that does not start on a dword (a slice of odd-sized frames) and a list of such frames are repacked by
    the Python layer, not refused by the C entry point's alignment check."""
    imgs = np.stack([rr.noise_image(30 + n, 5, 7) for n in range(5)])  # 105 bytes a frame
    t = torch.from_numpy(imgs).to(DEV)
    view = t[1:]
    assert view.is_contiguous() and view.data_ptr() % 4 != 0
    for frames in (view, list(view.unbind(0))):
        got = gd.resized_crop_frames(frames, size=(12, 20), T=2).cpu().numpy()
        for n in range(4):
            np.testing.assert_array_equal(got[n // 2, :, n % 2], rr.augment(imgs[n + 1], None, False, (12, 20), MEAN, STD))
    raw = torch.from_numpy(rr.noise_image(40, 1, 73).reshape(-1)).to(DEV)  # 219 bytes
    odd = raw[1:217].view(2, 6, 6, 3)  # frames of 108 bytes (whole dwords) that start one byte off a dword
    assert odd.is_contiguous() and odd.data_ptr() % 4 == 1
    got = gd.resized_crop_frames(odd, size=8).cpu().numpy()
    for n in range(2):
        np.testing.assert_array_equal(got[n, :, 0], rr.augment(odd[n].cpu().numpy(), None, False, 8, MEAN, STD))


def test_kernel_defends_itself_against_bad_descriptors():
    """What a C caller can get wrong in the descriptor table, which the entry point cannot see on the host: a box that overhangs
    its frame is clamped into it; a frame that does not lie inside src, and a box too large for the kernel's LDS, come out as NaN.
    Nothing is read out of bounds (the kernel checks before it reads), and the neighbouring images of the launch are right."""
    small = [rr.noise_image(60 + n, 64, 80) for n in range(5)]
    wide = rr.noise_image(66, 4, 60000)
    assert L.load().gdl_frames_resized_crop_box_ok(4, 60000, 32, 40) == 0
    imgs = small + [wide]

    def edit(rows):
        rows[0][3:7] = [20, 30, 100, 100]   # overhangs bottom and right  -> (20, 30, 44, 50)
        rows[1][3:7] = [-3, -9, 0, 0]       # negative corner, empty box  -> (0, 0, 1, 1)
        rows[2][3:7] = [70, 90, 5, 5]       # corner outside the frame    -> (63, 79, 1, 1)
        rows[3][0] = 1 << 40                # the frame is not inside src -> NaN
        # rows[4]: untouched; rows[5]: the whole 4 x 60000 frame, which does not fit -> NaN

    got = _call_abi(imgs, [None] * 6, [False, True, False, False, True, False], 6, 1, 32, 40, edit=edit).cpu().numpy()[:, :, 0]
    np.testing.assert_array_equal(got[0], rr.augment(small[0], (20, 30, 44, 50), False, (32, 40), MEAN, STD))
    np.testing.assert_array_equal(got[1], rr.augment(small[1], (0, 0, 1, 1), True, (32, 40), MEAN, STD))
    np.testing.assert_array_equal(got[2], rr.augment(small[2], (63, 79, 1, 1), False, (32, 40), MEAN, STD))
    assert np.isnan(got[3]).all() and np.isnan(got[5]).all()
    np.testing.assert_array_equal(got[4], rr.augment(small[4], None, True, (32, 40), MEAN, STD))
    # a frame whose end lies past src_bytes by one byte
    def short(rows):
        rows[1][1] += 1  # one more row than the buffer holds

    got = _call_abi(small[:2], [None] * 2, [False] * 2, 2, 1, 32, 40, edit=short).cpu().numpy()[:, :, 0]
    np.testing.assert_array_equal(got[0], rr.augment(small[0], None, False, (32, 40), MEAN, STD))
    assert np.isnan(got[1]).all()


def test_errors_are_raised_on_the_host():
    """Every check happens before a launch: the output buffer keeps its fill."""
    img = rr.noise_image(1, 32, 32)
    with pytest.raises(L.GdlError, match="B \\* T"):
        _call_abi([img] * 4, [None] * 4, [False] * 4, 2, 2, 16, 16, n_img=3)
    for oh, ow in ((0, 16), (16, 0)):
        src = torch.zeros(64, dtype=torch.uint8, device=DEV)
        desc = torch.zeros(8, dtype=torch.int64, device=DEV)
        out = torch.full((64,), 7.0, device=DEV)
        m = (ctypes.c_float * 3)(*MEAN)
        with pytest.raises(L.GdlError, match="must be positive"):
            L.call("gdl_frames_resized_crop", L.ptr(src), 64, L.ptr(desc), 1, 1, 1, oh, ow, ctypes.cast(m, ctypes.c_void_p),
                   ctypes.cast(m, ctypes.c_void_p), L.ptr(out), L.cur_stream())
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    with pytest.raises(L.GdlError, match="zero std"):
        _call_abi([img], [None], [False], 1, 1, 16, 16, std=(0.2, 0.0, 0.2))
    frames = torch.from_numpy(img).to(DEV)[None]
    for kw in (dict(boxes=[(0, 0, 33, 32)]), dict(boxes=[(0, 0, 0, 32)]), dict(boxes=[(30, 30, 4, 4)]), dict(T=2),
               dict(flips=[True, False]), dict(out=torch.empty(1, 3, 1, 8, 8, device=DEV))):
        with pytest.raises(ValueError):
            gd.resized_crop_frames(frames, **kw)
    with pytest.raises(ValueError):
        gd.resized_crop_frames(frames.float())
