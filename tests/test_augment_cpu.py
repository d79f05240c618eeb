"""CPU-only checks of the device-side frame augmentation (gdl.data.resized_crop_frames / gdl_frames_resized_crop): the NumPy
restatement the GPU tests hold the kernel to bit for bit (tests/resize_ref.py, Pillow's bilinear ImagingResample) is measured
against an independent implementation that is installed -- torch's antialiased CPU resize; the box draws follow torchvision's
published RandomResizedCrop.get_params; the argument errors and the C ABI need no device."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resize_ref as rr  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gdl import data as gd  # noqa: E402

# Share of differing pixels recorded in docs/parity_log.md (tools/resize_parity.py, torch 2.10): case -> (uint8 path, float32 path
# rounded to uint8).  The uint8 figures are the same for contiguous and channels_last input.
RECORDED = {
    "down_360x480_box": (0.004252, 0.169816),
    "down_1080x1920_box": (0.001183, 0.086648),
    "up_37x53": (0.001946, 0.189247),
    "each_way_224x500": (0.011021, 0.194921),
    "identity_rows_224x500": (0.001016, 0.000512),
    "identity_cols_500x224": (0.000957, 0.000578),
    "whole_360x480": (0.000977, 0.156283),
    "one_pixel_wide": (0.010417, 0.013393),
    "one_pixel_high": (0.004464, 0.007440),
    "nonsquare_160x288": (0.009122, 0.140647),
    "odd_out_97x131_up_down": (0.001259, 0.137955),
}


@pytest.mark.parametrize("i", range(len(rr.CASES)), ids=[c[0] for c in rr.CASES])
def test_restatement_against_torch_antialiased_resize(i):
    """resize_ref.resized_crop_u8 against F.interpolate(uint8 CPU, mode="bilinear", antialias=True) of the cropped tensor.  What
    is measured is the restatement, never the kernel.

    Recorded (docs/parity_log.md): on seeded noise the largest difference is 1 grey level in every case and on every path.  The
    restatement matches torch's uint8 path best -- 0.1 % to 1.1 % of the pixels differ (contiguous and channels_last give the same
    figures), against 9 % to 19 % for the float32 path rounded to uint8, which has no uint8 intermediate.  On a smooth image the
    mean absolute difference is at most 0.0002 level (uint8 paths) and 0.19 level (float32 path).

    Bounds: max |diff| <= 2 (two implementations of the same two-pass filter with differently rounded coefficients can differ by
    one level in the uint8 intermediate, a normalised vertical filter carries that through as at most one level, the second
    rounding can add one more); share of differing pixels under twice the recorded one; smooth image below 0.5 level."""
    case = rr.CASES[i]
    assert set(RECORDED) == {c[0] for c in rr.CASES}
    for path in rr.PATHS:
        mx, share, _ = rr.measure(i, case, path)
        recorded = RECORDED[case[0]][path == "f32_rounded"]
        print(f"{case[0]} {path}: max {mx}, share {share:.6f} (recorded {recorded:.6f})")
        assert mx <= 2, (path, mx)
        assert share < 2 * recorded, (path, share, recorded)
        mean_abs = rr.measure(i, case, path, smooth=True)[2]
        print(f"{case[0]} {path}: smooth image, mean abs diff {mean_abs:.4f}")
        assert mean_abs < 0.5, (path, mean_abs)


def test_restatement_basics():
    """Things the algorithm guarantees on its own: equal sizes are the identity, coefficients sum to 2^22 up to rounding, the taps
    stay inside the input, a constant image stays constant, the flip mirrors the resized image, the normalise is
    test_normalize_frames' expression."""
    img = rr.noise_image(3, 40, 56)
    np.testing.assert_array_equal(rr.resized_crop_u8(img, None, 40, 56), img)
    np.testing.assert_array_equal(rr.resized_crop_u8(img, (4, 5, 20, 30), 20, 30), img[4:24, 5:35])
    for n_in, n_out in ((480, 224), (37, 224), (1, 224), (1920, 224), (224, 224), (85, 131)):
        for xmin, k in rr.coeffs(n_in, n_out):
            assert 0 <= xmin and xmin + len(k) <= n_in and len(k) >= 1 and (k >= 0).all()
            assert len(k) <= 2 * max(1, math.ceil(n_in / n_out)) + 1
            assert abs(int(k.sum()) - (1 << 22)) <= len(k)
    flat = np.full((50, 70, 3), 201, np.uint8)
    assert (rr.resized_crop_u8(flat, (1, 2, 45, 60), 24, 31) == 201).all()
    a = rr.augment(img, (4, 5, 20, 30), False, (24, 18), gd.IMAGENET_MEAN, gd.IMAGENET_STD)
    b = rr.augment(img, (4, 5, 20, 30), True, (24, 18), gd.IMAGENET_MEAN, gd.IMAGENET_STD)
    assert a.shape == (3, 24, 18) and a.dtype == np.float32
    np.testing.assert_array_equal(b, a[:, :, ::-1])
    t = torch.from_numpy(rr.resized_crop_u8(img, (4, 5, 20, 30), 24, 18)).permute(2, 0, 1).float().div(255.0)
    want = (t - torch.tensor(gd.IMAGENET_MEAN).view(3, 1, 1)) / torch.tensor(gd.IMAGENET_STD).view(3, 1, 1)
    np.testing.assert_array_equal(a, want.numpy())


SCALE, RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)


@pytest.mark.parametrize("size", [(360, 480), (224, 224), (1080, 1920)])
def test_random_resized_crop_params_ranges(size):
    """10 000 seeded draws: every box inside its frame, area and ratio inside the ranges up to the rounding of one pixel a side."""
    H, W = size
    g = torch.Generator().manual_seed(7)
    boxes = gd.random_resized_crop_params([size] * 10000, generator=g)
    assert boxes.dtype == torch.int64 and tuple(boxes.shape) == (10000, 4)
    top, left, h, w = (boxes[:, k].double() for k in range(4))
    assert bool((top >= 0).all() and (left >= 0).all() and (h >= 1).all() and (w >= 1).all())
    assert bool((top + h <= H).all() and (left + w <= W).all())
    # w = round(sqrt(a r)), h = round(sqrt(a / r)) for some a in area * scale, r in ratio: each side is within half a pixel of
    # its real value, so the real box lies between (w - 1/2, h - 1/2) and (w + 1/2, h + 1/2)
    area = float(H * W)
    assert bool(((w + 0.5) * (h + 0.5) >= SCALE[0] * area).all() and ((w - 0.5) * (h - 0.5) <= SCALE[1] * area).all())
    assert bool(((w + 0.5) / (h - 0.5) >= RATIO[0]).all() and ((w - 0.5) / (h + 0.5) <= RATIO[1]).all())
    assert len({tuple(b) for b in boxes.tolist()}) > 9000  # they are draws, not one box
    again = gd.random_resized_crop_params([size] * 100, generator=torch.Generator().manual_seed(7))
    assert torch.equal(again, boxes[:100])  # same seed, same boxes


def test_random_resized_crop_params_follow_the_published_algorithm():
    """gd.random_resized_crop_params draws what resize_ref.rrc_params (restated from the publication) computes from the same
    uniform numbers in the same order; the fallback after ten refused tries is the central crop clamped to the ratio range."""
    sizes = [(360, 480), (224, 224), (100, 37), (1080, 1920)] * 50
    got = gd.random_resized_crop_params(sizes, generator=torch.Generator().manual_seed(3))
    g = torch.Generator().manual_seed(3)
    uniform = lambda a, b: torch.empty(1).uniform_(float(a), float(b), generator=g).item()  # noqa: E731
    randint = lambda n: torch.randint(0, n, size=(1,), generator=g).item()  # noqa: E731
    want = [rr.rrc_params(h, w, SCALE, RATIO, uniform, randint) for h, w in sizes]
    assert got.tolist() == [list(b) for b in want]
    # injected source: always the largest area and the widest ratio -> a 100 x 100 frame cannot hold round(sqrt(10^4 * 4/3)) = 115
    # columns, ten times; the frame's own ratio is inside the range, so the fallback is the whole frame
    calls = []

    def top_of_range(a, b):
        calls.append((a, b))
        return b

    def no_randint(n):
        raise AssertionError("the fallback draws no position")

    assert rr.rrc_params(100, 100, SCALE, RATIO, top_of_range, no_randint) == (0, 0, 100, 100)
    assert len(calls) == 20
    assert rr.rrc_params(100, 400, SCALE, RATIO, top_of_range, no_randint) == (0, 133, 100, 133)  # too wide: h = H, w = round(H * 4/3)
    assert rr.rrc_params(400, 100, SCALE, RATIO, top_of_range, no_randint) == (133, 0, 133, 100)  # too tall: w = W, h = round(W / (3/4))
    # the same branch in gd: a 10 x 1000 frame with scale >= 0.9 never fits a box of ratio <= 4/3
    b = gd.random_resized_crop_params([(10, 1000), (1000, 10)], scale=(0.9, 1.0), generator=torch.Generator().manual_seed(0))
    assert b.tolist() == [[0, 493, 10, 13], [493, 0, 13, 10]]
    f = gd.random_flips(10000, generator=torch.Generator().manual_seed(1))
    assert f.dtype == torch.bool and 4700 < int(f.sum()) < 5300
    assert torch.equal(f[:50], gd.random_flips(50, generator=torch.Generator().manual_seed(1)))
    assert not gd.random_flips(20, p=0.0).any() and gd.random_flips(20, p=1.0).all()


def test_random_augment_params_interleave_like_compose():
    """Compose([RandomResizedCrop, RandomHorizontalFlip]) runs per image, so the random stream is box, flip, box, flip, ...:
    random_augment_params equals that sequence drawn by hand from the same seed, and differs from all boxes then all flips."""
    sizes = [(360, 480), (100, 37), (224, 224)] * 20
    boxes, flips = gd.random_augment_params(sizes, generator=torch.Generator().manual_seed(9))
    g = torch.Generator().manual_seed(9)
    uniform = lambda a, b: torch.empty(1).uniform_(float(a), float(b), generator=g).item()  # noqa: E731
    randint = lambda n: torch.randint(0, n, size=(1,), generator=g).item()  # noqa: E731
    for n, (h, w) in enumerate(sizes):
        assert tuple(boxes[n].tolist()) == rr.rrc_params(h, w, SCALE, RATIO, uniform, randint), n
        assert bool(flips[n]) == (torch.rand(1, generator=g).item() < 0.5), n
    assert boxes.dtype == torch.int64 and flips.dtype == torch.bool and 15 < int(flips.sum()) < 45
    g = torch.Generator().manual_seed(9)
    assert not torch.equal(gd.random_resized_crop_params(sizes, generator=g), boxes)


def test_argument_errors_need_no_device():
    host = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for fn in (lambda: gd.resized_crop_frames(host),                      # a host tensor: there is no CPU path
               lambda: gd.resized_crop_frames([host[0], host[1]]),
               lambda: gd.resized_crop_frames(host.float()),             # not uint8
               lambda: gd.augment_frames(host, 1, True),
               lambda: gd.augment_frames(host, 1, False),
               lambda: gd.resized_crop_frames(host, size=0)):
        with pytest.raises(ValueError):
            fn()
    sizes = [(8, 8)] * 6
    desc, nbytes, B = gd.crop_descriptors(sizes, None, None, 3, 224)
    assert B == 2 and nbytes == 6 * 192 and desc.dtype == torch.int64
    assert desc.tolist() == [[192 * i, 8, 8, 0, 0, 8, 8, 0] for i in range(6)]
    desc, nbytes, _ = gd.crop_descriptors([(3, 3), (5, 7)], [(0, 1, 2, 2), (1, 1, 4, 6)], [True, False], 1, (16, 24))
    assert desc.tolist() == [[0, 3, 3, 0, 1, 2, 2, 1], [28, 5, 7, 1, 1, 4, 6, 0]] and nbytes == 28 + 108  # frames start on dwords
    ok = [(0, 0, 8, 8)] * 6
    for boxes in ([(0, 0, 9, 8)] + ok[1:], [(1, 0, 8, 8)] + ok[1:], ok[:5] + [(0, 4, 8, 5)], ok[:5] + [(0, 0, 0, 8)],
                  ok[:5] + [(0, 0, 8, 0)], [(-1, 0, 4, 4)] + ok[1:], ok[:5]):
        with pytest.raises(ValueError):
            gd.crop_descriptors(sizes, boxes, None, 3, 224)
    with pytest.raises(ValueError):
        gd.crop_descriptors(sizes, None, None, 4, 224)      # 6 frames are not B * 4
    with pytest.raises(ValueError):
        gd.crop_descriptors(sizes, None, [True] * 5, 3, 224)
    with pytest.raises(ValueError):
        gd.crop_descriptors([], None, None, 1, 224)
    with pytest.raises(ValueError, match="does not fit"):      # the documented limit: a box far wider than the tables hold
        gd.crop_descriptors([(100, 60000)], None, None, 1, 224)
    gd.crop_descriptors([(1080, 1920)], None, None, 1, 224)   # a full-HD frame fits


def test_abi_has_the_entry_point():
    src = open(os.path.join(ROOT, "include", "gdl_hip.h")).read()
    lib = ctypes.CDLL(L.SO_PATH)  # loads without a GPU
    for name in ("gdl_frames_resized_crop", "gdl_frames_resized_crop_box_ok"):
        assert f"GDL_API int {name}(" in src, name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    assert L.SIGNATURES["gdl_frames_resized_crop"] == ("i", "pzp" + "iiiii" + "ppp" + "p")
    lib = L.load()
    assert lib.gdl_frames_resized_crop_box_ok(360, 480, 224, 224) == 1
    assert lib.gdl_frames_resized_crop_box_ok(1080, 1920, 224, 224) == 1
    assert lib.gdl_frames_resized_crop_box_ok(1, 1, 224, 224) == 1
    assert lib.gdl_frames_resized_crop_box_ok(0, 10, 224, 224) == 0
    assert lib.gdl_frames_resized_crop_box_ok(100, 60000, 224, 224) == 0
    # the host checks come before anything touches a device: no GPU is needed to be refused
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    std = (ctypes.c_float * 3)(0.5, 0.0, 0.5)
    buf = ctypes.create_string_buffer(64)
    rc = lib.gdl_frames_resized_crop(ctypes.addressof(buf), 64, ctypes.addressof(buf), 3, 1, 2, 8, 8, ctypes.cast(mean, ctypes.c_void_p),
                                     ctypes.cast(mean, ctypes.c_void_p), ctypes.addressof(buf), None)
    assert rc != 0 and b"B * T" in lib.gdl_last_error()
    rc = lib.gdl_frames_resized_crop(ctypes.addressof(buf), 64, ctypes.addressof(buf), 2, 1, 2, 8, 8, ctypes.cast(mean, ctypes.c_void_p),
                                     ctypes.cast(std, ctypes.c_void_p), ctypes.addressof(buf), None)
    assert rc != 0 and b"zero std" in lib.gdl_last_error()
