"""Device-side stages of the reference's input pipeline over gdl_logspec / gdl_frames_normalize /
gdl_frames_resized_crop.

The reference computes all of them per sample on DataLoader workers (dataset/CramedDataset.py:58-95, KSDataset.py:136-190,
VGGSoundDataset.py:110-160): a log-magnitude librosa STFT of the clipped waveform, and RandomResizedCrop(224) +
RandomHorizontalFlip + ToTensor + Normalize (training) or Resize((224, 224)) + ToTensor + Normalize (evaluation) of the decoded
frames.  Here a whole batch is one kernel launch each.  What stays on the host: file decoding, resampling and tiling / cropping
of the waveform, decoding the frames to uint8, and drawing the crop boxes and flips -- a few integers per frame
(random_augment_params); everything that touches a pixel runs on the device.

Nothing is computed on the CPU: the functions that produce tensors need device tensors and the built library.
"""
import ctypes
import math

import torch

from . import _lib as L

PAD_MODES = {"constant": 0, "reflect": 1}  # GDL_PAD_CONSTANT / GDL_PAD_REFLECT
IMAGENET_MEAN = (0.485, 0.456, 0.406)      # the constants of every dataset of the reference
IMAGENET_STD = (0.229, 0.224, 0.225)

# (n_fft, hop_length) of the reference's datasets
STFT_CREMAD = (512, 353)   # CramedDataset.py:65 -> [257, 188] for 3 s at 22 050 Hz
STFT_KS = (256, 128)       # KSDataset.py:148, VGGSoundDataset.py:121 -> [129, 626] for 5 s at 16 kHz
STFT_AVE = (512, 256)      # AVEDataset.py:86, Audioset.py:149


def log_spectrogram(wave, n_fft=512, hop_length=353, pad_mode="constant", out=None):
    """`np.log(np.abs(librosa.stft(clip(wave, -1, 1), n_fft=n_fft, hop_length=hop_length)) + 1e-7)` for a batch.

    wave: float32 device tensor [B, n_samples] (or [n_samples]); returns float32 [B, n_fft//2+1, 1 + n_samples//hop]
    -- `spec` as main_dgl.py:108 receives it (it adds the channel axis itself).  pad_mode is librosa's: 'constant'
    (librosa >= 0.10, zeros) or 'reflect' (older releases); the reference does not pin a librosa version."""
    if pad_mode not in PAD_MODES:
        raise ValueError(f"gdl: pad_mode must be one of {sorted(PAD_MODES)}, not {pad_mode!r}")
    squeeze = wave.dim() == 1
    w = wave.reshape(1, -1) if squeeze else wave
    if w.dim() != 2 or w.dtype != torch.float32 or not w.is_cuda:
        raise ValueError("gdl: wave must be a float32 device tensor [B, n_samples]")
    w = w.contiguous()
    B, n = w.shape
    frames = L.load().gdl_logspec_frames(n, hop_length)
    if out is None:
        out = torch.empty(B, n_fft // 2 + 1, frames, dtype=torch.float32, device=w.device)
    elif tuple(out.shape) != (B, n_fft // 2 + 1, frames) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("gdl: out must be a contiguous float32 tensor [B, n_fft//2+1, frames]")
    L.call("gdl_logspec", L.ptr(w), B, n, n_fft, hop_length, PAD_MODES[pad_mode], L.ptr(out), L.cur_stream())
    return out[0] if squeeze else out


def normalize_frames(frames_u8, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """transforms.ToTensor() + transforms.Normalize(mean, std) for a stack of decoded frames.

    frames_u8: uint8 device tensor [..., H, W, 3] (e.g. [B, T, 224, 224, 3]); returns float32 [..., 3, H, W]."""
    f = frames_u8
    if f.dtype != torch.uint8 or not f.is_cuda or f.dim() < 3 or f.shape[-1] != 3:
        raise ValueError("gdl: frames must be a uint8 device tensor [..., H, W, 3]")
    f = f.contiguous()
    lead, (H, W) = tuple(f.shape[:-3]), f.shape[-3:-1]
    n_img = 1
    for d in lead:
        n_img *= d
    if out is None:
        out = torch.empty(*lead, 3, H, W, dtype=torch.float32, device=f.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    L.call("gdl_frames_normalize", L.ptr(f), n_img, H, W, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p),
           L.ptr(out), L.cur_stream())
    return out


def random_resized_crop_params(sizes, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """torchvision's published RandomResizedCrop.get_params for a list of (H, W) frame sizes; int64 tensor [n, 4] of
    (top, left, height, width) on the host.

    Per frame, up to 10 tries of: area * U(scale), exp(U(log ratio)) (float32, as published), w = round(sqrt(a * r)),
    h = round(sqrt(a / r)); accepted if it fits the frame, then top and left uniform; otherwise the central crop clamped to the
    ratio range.  torch's RNG in get_params' draw order (area factor, log-ratio, top, left), so that a maintainer can line it up
    with torchvision's get_params where that is installed; it is not installed with this project, so that has not been checked.
    The datasets' Compose draws a flip after each frame's box: random_augment_params has that order."""
    log_ratio = torch.log(torch.tensor(ratio))
    boxes = torch.empty(len(sizes), 4, dtype=torch.int64)
    for n, (height, width) in enumerate(sizes):
        height, width = int(height), int(width)
        if height < 1 or width < 1:
            raise ValueError(f"gdl: frame size ({height}, {width}) must be positive")
        area = height * width
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
            aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)).item()
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if 0 < w <= width and 0 < h <= height:
                top = torch.randint(0, height - h + 1, size=(1,), generator=generator).item()
                left = torch.randint(0, width - w + 1, size=(1,), generator=generator).item()
                break
        else:
            in_ratio = float(width) / float(height)
            if in_ratio < min(ratio):
                w = width
                h = int(round(w / min(ratio)))
            elif in_ratio > max(ratio):
                h = height
                w = int(round(h * max(ratio)))
            else:
                w, h = width, height
            top, left = (height - h) // 2, (width - w) // 2
        boxes[n] = torch.tensor([top, left, h, w])
    return boxes


def random_flips(n, p=0.5, generator=None):
    """RandomHorizontalFlip(p) for n frames: one `torch.rand(1) < p` per frame, as published; bool tensor [n] on the host."""
    return torch.tensor([torch.rand(1, generator=generator).item() < p for _ in range(n)], dtype=torch.bool)


def _size2(size):
    out_h, out_w = (size, size) if isinstance(size, int) else size
    if int(out_h) < 1 or int(out_w) < 1:
        raise ValueError(f"gdl: output size {size!r} must be positive")
    return int(out_h), int(out_w)


def _frame_list(frames):
    """-> (list of [H_i, W_i, 3] views, the stacked tensor or None)."""
    if isinstance(frames, torch.Tensor):
        f = frames
        if f.dtype != torch.uint8 or not f.is_cuda or f.dim() < 3 or f.shape[-1] != 3:
            raise ValueError("gdl: frames must be a uint8 device tensor [..., H, W, 3] or a list of uint8 device tensors [H, W, 3]")
        f = f.contiguous().reshape(-1, f.shape[-3], f.shape[-2], 3)
        return list(f.unbind(0)), f
    fl = list(frames)
    for f in fl:
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or not f.is_cuda or f.dim() != 3 or f.shape[-1] != 3:
            raise ValueError("gdl: frames must be a uint8 device tensor [..., H, W, 3] or a list of uint8 device tensors [H, W, 3]")
    return fl, None


def crop_descriptors(sizes, boxes=None, flips=None, T=1, size=224):
    """The host half of resized_crop_frames: checks the boxes of frames of `sizes` [(H, W)] and lays the frames out in one packed
    buffer.  Returns (desc, nbytes, B): the int64 [n, 8] table gdl_frames_resized_crop reads (byte offset, H, W, top, left, box
    height, box width, flip), the length of the packed buffer (every frame starts on a dword) and the batch size n / T.
    Raises ValueError for a box that is empty, not inside its frame or too large for the kernel, and for n != B * T."""
    out_h, out_w = _size2(size)
    n, T = len(sizes), int(T)
    if n == 0 or T < 1 or n % T != 0:
        raise ValueError(f"gdl: {n} frames are not B * T frames for T = {T}")
    if boxes is None:
        boxes = [(0, 0, h, w) for h, w in sizes]
    boxes = torch.as_tensor(boxes, dtype=torch.int64, device="cpu").reshape(-1, 4)
    flips = torch.zeros(n, dtype=torch.bool) if flips is None else torch.as_tensor(flips, device="cpu").reshape(-1).bool()
    if boxes.shape[0] != n or flips.shape[0] != n:
        raise ValueError(f"gdl: {n} frames need {n} boxes and flips, not {boxes.shape[0]} and {flips.shape[0]}")
    lib = L.load()
    rows, offset = [], 0
    for i, ((h, w), (top, left, bh, bw), flip) in enumerate(zip(sizes, boxes.tolist(), flips.tolist())):
        if bh < 1 or bw < 1 or top < 0 or left < 0 or top + bh > h or left + bw > w:
            raise ValueError(f"gdl: box {(top, left, bh, bw)} of frame {i} is empty or not inside its {h} x {w} frame")
        if not lib.gdl_frames_resized_crop_box_ok(bh, bw, out_h, out_w):
            raise ValueError(f"gdl: box {(top, left, bh, bw)} of frame {i} -> {out_h} x {out_w} does not fit the kernel's 40 KB of "
                             "LDS (include/gdl_hip.h, gdl_frames_resized_crop: limits)")
        rows.append([offset, h, w, top, left, bh, bw, int(flip)])
        offset += (h * w * 3 + 3) // 4 * 4
    return torch.tensor(rows, dtype=torch.int64), offset, n // T


def resized_crop_frames(frames, boxes=None, flips=None, size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, T=1, out=None):
    """Crop each frame to its box, resize the crop to `size` with Pillow's antialiased bilinear filter (what transforms.Resize and
    RandomResizedCrop run on a PIL image), flip where asked, ToTensor + Normalize -- one launch for the batch.

    frames: one uint8 device tensor [..., H, W, 3] (all frames one size) or a list of uint8 device tensors [H_i, W_i, 3], B * T of
    them, frame t of sample b at index b * T + t.  boxes: [n, 4] integers (top, left, height, width) on the host, None = the whole
    frame, i.e. Resize((size, size)).  flips: [n] booleans, None = no flip.  size: int or (height, width).  Returns float32
    [B, 3, T, h, w], the `image` DGLTrainer.step and AVClassifier_DGL.forward take."""
    out_h, out_w = _size2(size)
    fl, stacked = _frame_list(frames)
    sizes = [(int(f.shape[0]), int(f.shape[1])) for f in fl]
    desc, nbytes, B = crop_descriptors(sizes, boxes, flips, T, (out_h, out_w))
    n, T = len(fl), int(T)
    dev = fl[0].device
    if stacked is not None and (sizes[0][0] * sizes[0][1] * 3) % 4 == 0 and stacked.data_ptr() % 4 == 0:
        src = stacked  # already packed at these offsets, and on a dword as the kernel's staging loads need
    else:  # one concatenation: the frames' bytes, each padded to a whole number of dwords (a fresh allocation is aligned)
        parts = []
        for f in fl:
            parts.append(f.reshape(-1))
            if f.numel() % 4:
                parts.append(torch.zeros(4 - f.numel() % 4, dtype=torch.uint8, device=dev))
        src = torch.cat(parts)
        assert src.numel() == nbytes
    if out is None:
        out = torch.empty(B, 3, T, out_h, out_w, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, 3, T, out_h, out_w) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("gdl: out must be a contiguous float32 device tensor [B, 3, T, h, w]")
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    L.call("gdl_frames_resized_crop", L.ptr(src), src.numel(), L.ptr(desc.to(dev)), n, B, T, out_h, out_w,
           ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), L.ptr(out), L.cur_stream())
    return out


def random_augment_params(sizes, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip=0.5, generator=None):
    """The draws of Compose([RandomResizedCrop, RandomHorizontalFlip]) applied frame by frame, as the datasets apply it: per
    frame the box (random_resized_crop_params' draws), then the flip (one torch.rand(1) < p), so the random stream interleaves
    box and flip like torchvision's.  Returns (boxes int64 [n, 4], flips bool [n]) on the host.  (Like the box draws, not
    checked against torchvision, which is not installed with this project.)"""
    boxes = torch.empty(len(sizes), 4, dtype=torch.int64)
    flips = torch.empty(len(sizes), dtype=torch.bool)
    for n, size in enumerate(sizes):
        boxes[n] = random_resized_crop_params([size], scale, ratio, generator)[0]
        flips[n] = random_flips(1, p_flip, generator)[0]
    return boxes, flips


def augment_frames(frames, T, train, generator=None, size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, scale=(0.08, 1.0),
                   ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip=0.5, out=None):
    """The two visual transforms of the reference's datasets by name (CramedDataset.py:76-88).  train=True:
    RandomResizedCrop(size) + RandomHorizontalFlip() + ToTensor() + Normalize -- box and flip are drawn frame by frame
    (random_augment_params) from `generator` (torch's global RNG if None).  train=False: Resize((size, size)) + ToTensor() +
    Normalize.  frames and the result as resized_crop_frames."""
    if not train:
        return resized_crop_frames(frames, None, None, size, mean, std, T, out)
    fl, _ = _frame_list(frames)
    boxes, flips = random_augment_params([(f.shape[0], f.shape[1]) for f in fl], scale, ratio, p_flip, generator)
    return resized_crop_frames(frames, boxes, flips, size, mean, std, T, out)
