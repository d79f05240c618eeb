"""NumPy restatement of the arithmetic behind gdl.data.resized_crop_frames / gdl_frames_resized_crop (csrc/input.hip).

The reference's datasets call transforms.RandomResizedCrop(224) / Resize((224, 224)) on PIL images, i.e. Pillow's
ImagingResample with the bilinear (triangle) filter; neither Pillow nor torchvision is installed with this project, so their
published algorithm is restated here and pinned to torch.nn.functional.interpolate(uint8, antialias=True) in
test_augment_cpu.py.  Everything on pixels is integer arithmetic, so the device result has to equal this bit for bit.

  * crop first (img.crop), then resize the crop: pixels outside the box never contribute;
  * separable, horizontal pass first, then vertical, the intermediate image rounded to uint8;
  * per output index i of a pass in -> out:  scale = in / out, filterscale = max(1, scale), support = filterscale,
    center = (i + 0.5) * scale, xmin = max(0, int(center - support + 0.5)), xmax = min(in, int(center + support + 0.5)),
    w[x] = triangle((x - center + 0.5) / filterscale) for x in [xmin, xmax), normalised to sum 1 in double precision,
    k[x] = int(0.5 + w[x] * 2**22);  out = clip((2**21 + sum_x k[x] * pixel[x]) >> 22, 0, 255).
    The order of the double-precision operations is Pillow's (precompute_coeffs: `(x + xmin - center + 0.5) * ss` with
    ss = 1 / filterscale, the weights summed in tap order, each divided by the sum).

No GPU, no import of the reference.  (torch is imported only by the comparison helpers at the end.)
"""
import math

import numpy as np

PRECISION_BITS = 22  # Pillow: 32 - 8 - 2


def coeffs(in_size, out_size):
    """Per output index: (xmin, int32 coefficients of the taps xmin .. xmin + len)."""
    scale = float(in_size) / float(out_size)
    filterscale = scale if scale > 1.0 else 1.0
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = []
        ww = 0.0
        for x in range(xmax - xmin):
            v = (x + xmin - center + 0.5) * ss
            v = -v if v < 0.0 else v
            v = 1.0 - v if v < 1.0 else 0.0
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, np.array([int(0.5 + v * (1 << PRECISION_BITS)) for v in w], np.int64)))
    return out


def _pass(img, out_size, axis):
    """One pass along `axis` (0 rows, 1 columns) of a uint8 [h, w, c] image."""
    img = np.moveaxis(img, axis, 0)
    res = np.empty((out_size,) + img.shape[1:], np.uint8)
    for i, (xmin, k) in enumerate(coeffs(img.shape[0], out_size)):
        acc = np.tensordot(k, img[xmin:xmin + len(k)].astype(np.int64), axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        res[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(res, 0, axis)


def resized_crop_u8(img, box, out_h, out_w):
    """img: uint8 [H, W, 3]; box: (top, left, height, width) or None for the whole frame.  Returns uint8 [out_h, out_w, 3]."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    if box is not None:
        top, left, h, w = (int(v) for v in box)
        assert 0 <= top and 0 <= left and h > 0 and w > 0 and top + h <= img.shape[0] and left + w <= img.shape[1], box
        img = img[top:top + h, left:left + w]
    if img.shape[1] != out_w:  # a pass whose input and output length are equal is skipped
        img = _pass(img, out_w, 1)
    if img.shape[0] != out_h:
        img = _pass(img, out_h, 0)
    return np.ascontiguousarray(img)


def normalize(u8_hwc, mean, std):
    """ToTensor + Normalize: ((x / 255) - mean[c]) / std[c] in that order of float32 operations; returns float32 CHW."""
    x = np.transpose(u8_hwc, (2, 0, 1)).astype(np.float32) / np.float32(255.0)
    m = np.asarray(mean, np.float32).reshape(3, 1, 1)
    s = np.asarray(std, np.float32).reshape(3, 1, 1)
    return ((x - m) / s).astype(np.float32)


def augment(img, box, flip, size, mean, std):
    """RandomResizedCrop's resize of `box`, RandomHorizontalFlip's flip if `flip`, ToTensor, Normalize.  size: int or (h, w)."""
    out_h, out_w = (size, size) if isinstance(size, int) else size
    u8 = resized_crop_u8(img, box, out_h, out_w)
    if flip:
        u8 = u8[:, ::-1]
    return normalize(u8, mean, std)


def rrc_params(height, width, scale, ratio, uniform, randint):
    """torchvision's published RandomResizedCrop.get_params for one (height, width) frame.  uniform(a, b) -> float in [a, b],
    randint(n) -> int in [0, n); draw order as published: per try the area factor, then the log-ratio, and on acceptance
    top then left.  The log-ratio bounds and the exponential are float32 there (torch.log(torch.tensor(ratio)))."""
    area = height * width
    lo, hi = (float(np.log(np.float32(r))) for r in ratio)
    for _ in range(10):
        target_area = area * uniform(scale[0], scale[1])
        aspect = float(np.exp(np.float32(uniform(lo, hi))))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            top = randint(height - h + 1)
            left = randint(width - w + 1)
            return top, left, h, w
    in_ratio = float(width) / float(height)  # fallback: the central crop, clamped to the ratio range
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


# ---------------------------------------------------------------- the cases of test_augment_cpu.py / test_augment_gpu.py
# (name, source H, source W, box (top, left, height, width) or None = whole frame, out_h, out_w)
CASES = [
    ("down_360x480_box", 360, 480, (23, 41, 300, 400), 224, 224),       # downscale on both axes
    ("down_1080x1920_box", 1100, 1940, (11, 13, 1080, 1920), 224, 224),  # factors 4.8 / 8.6
    ("up_37x53", 37, 53, None, 224, 224),                               # upscale on both
    ("each_way_224x500", 224, 500, (10, 0, 120, 500), 224, 224),        # rows up, columns down
    ("identity_rows_224x500", 224, 500, None, 224, 224),                # the vertical pass is skipped
    ("identity_cols_500x224", 500, 224, None, 224, 224),                # the horizontal pass is skipped
    ("whole_360x480", 360, 480, None, 224, 224),                        # box = whole frame (the evaluation transform)
    ("one_pixel_wide", 64, 64, (5, 7, 40, 1), 224, 224),
    ("one_pixel_high", 64, 64, (5, 7, 1, 40), 224, 224),
    ("nonsquare_160x288", 360, 480, (23, 41, 300, 400), 160, 288),      # an output that is neither square nor 224
    ("odd_out_97x131_up_down", 200, 90, (3, 2, 190, 85), 97, 131),      # rows down, columns up, odd sizes
]


def noise_image(seed, H, W):
    """Seeded uniform noise: the worst case for rounding ties."""
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def smooth_image(seed, H, W):
    """A seeded low-frequency gradient: a half-pixel shift or a missing antialias shows here where noise hides it."""
    rng = np.random.default_rng(seed)
    y = np.linspace(0.0, 1.0, H)[:, None, None]
    x = np.linspace(0.0, 1.0, W)[None, :, None]
    a, b, p = rng.uniform(0.5, 1.5, 3), rng.uniform(0.5, 1.5, 3), rng.uniform(0.0, 6.28, 3)
    v = 127.5 + 80.0 * np.sin(2 * np.pi * (a * x + b * y) + p) + 40.0 * (x - y)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def case_image(i, case, smooth=False):
    _, H, W = case[:3]
    return (smooth_image if smooth else noise_image)(1000 + i, H, W)


def crop(img, box):
    if box is None:
        return img
    t, l, h, w = box
    return img[t:t + h, l:l + w]


# ---------------------------------------------------------------- the comparison with PyTorch's CPU resize
# (test_augment_cpu.py asserts on it, tools/resize_parity.py prints the table docs/parity_log.md records)
PATHS = ("u8_contiguous", "u8_channels_last", "f32_rounded")


def torch_resize(crop_hwc, out_h, out_w, path):
    """F.interpolate(mode="bilinear", antialias=True) of a uint8 HWC crop on the CPU: the uint8 path on contiguous or on
    channels_last input (separate code paths in PyTorch), or the float32 path rounded to uint8.  Returns uint8 HWC."""
    import torch
    import torch.nn.functional as F

    x = torch.from_numpy(np.ascontiguousarray(crop_hwc)).permute(2, 0, 1)[None]  # NCHW view of HWC memory = channels_last
    if path == "u8_contiguous":
        y = F.interpolate(x.contiguous(), size=(out_h, out_w), mode="bilinear", antialias=True)
    elif path == "u8_channels_last":
        y = F.interpolate(x.contiguous(memory_format=torch.channels_last), size=(out_h, out_w), mode="bilinear", antialias=True)
    else:
        y = F.interpolate(x.contiguous().float(), size=(out_h, out_w), mode="bilinear", antialias=True).round().clamp(0, 255).to(torch.uint8)
    return y[0].permute(1, 2, 0).contiguous().numpy()


def measure(i, case, path, smooth=False):
    """(max |diff|, share of differing pixels, mean |diff|) of the restatement against one PyTorch path."""
    _, _, _, box, oh, ow = case
    img = case_image(i, case, smooth)
    got = resized_crop_u8(img, box, oh, ow).astype(np.int32)
    want = torch_resize(crop(img, box), oh, ow, path).astype(np.int32)
    d = np.abs(got - want)
    return int(d.max()), float((d != 0).mean()), float(d.mean())
