"""Device-side stages of the reference's input pipeline over gdl_logspec / gdl_wave_logspec /
gdl_frames_normalize / gdl_frames_resized_crop.

The reference computes all of them per sample on DataLoader workers (dataset/CramedDataset.py:58-95, KSDataset.py:136-190,
VGGSoundDataset.py:110-160): librosa.load's PCM scale and mono mix-down, the tiling and the (random) window of the waveform, a
log-magnitude librosa STFT of the clipped window, and RandomResizedCrop(224) + RandomHorizontalFlip + ToTensor + Normalize
(training) or Resize((224, 224)) + ToTensor + Normalize (evaluation) of the decoded frames.  Here a whole batch is one kernel
launch each (wave_log_spectrogram / stage_audio, resized_crop_frames / augment_frames).  What stays on the host: decoding the
files to PCM samples and uint8 frames, resampling the audio of the 22050 Hz datasets (CREMA-D, AVE; the 16 kHz datasets' files
are stored at their rate), and drawing the window starts, the crop boxes and the flips -- a few integers per sample
(random_wave_starts, random_augment_params); everything that touches a sample's or a pixel's value runs on the device.
gdl.loader (DeviceDataset, DeviceLoader) draws them on the device too, for a dataset that lives there.

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


# ------------------------------------------------------------------ waveform staging (gdl_wave_logspec)
GDL_WAVE_F32, GDL_WAVE_S16 = 0, 1  # include/gdl_hip.h
_WAVE_FORMATS = {torch.float32: GDL_WAVE_F32, torch.int16: GDL_WAVE_S16}
_WAVE_BYTES = {GDL_WAVE_F32: 4, GDL_WAVE_S16: 2}

# The audio half of the reference datasets' __getitem__ as data.  rate: what librosa.load is asked for; tiling: ("times", 3) is
# np.tile(samples, 3), ("double", m) is `while len(sample) < m: sample = np.tile(sample, 2)` (m = 10 s); start_high: the window
# starts at random.randint(0, start_high), 0 = at the first sample, nothing drawn; n_samples: the window; resize: np.resize of
# the log spectrogram, None = none.  (CramedDataset.py:60-66 / 155-163, AVEDataset.py:81-88, KSDataset.py:139-149,
# VGGSoundDataset.py:112-122, Kinect400.py:120-129, Audioset.py:140-153.)
AUDIO_STAGES = {
    "CREMAD": dict(rate=22050, n_samples=66150, tiling=("times", 3), start_high=0, n_fft=512, hop_length=353, resize=None),
    "CREMAD_swin": dict(rate=22050, n_samples=66150, tiling=("times", 3), start_high=0, n_fft=512, hop_length=353, resize=(224, 224)),
    "AVE": dict(rate=22050, n_samples=66150, tiling=("times", 3), start_high=0, n_fft=512, hop_length=256, resize=(224, 224)),
    "KineticSound": dict(rate=16000, n_samples=80000, tiling=("double", 160000), start_high=80000, n_fft=256, hop_length=128, resize=None),
    "VGGSound": dict(rate=16000, n_samples=80000, tiling=("double", 160000), start_high=80000, n_fft=256, hop_length=128, resize=None),
    "kinect400": dict(rate=16000, n_samples=128000, tiling=("double", 160000), start_high=32000, n_fft=256, hop_length=128, resize=None),
    "Audioset": dict(rate=16000, n_samples=80000, tiling=("double", 160000), start_high=80000, n_fft=512, hop_length=256, resize=(224, 224)),
}


def wave_limit(length, tiling):
    """The length of a clip of `length` samples after a dataset's tiling (AUDIO_STAGES[name]["tiling"])."""
    kind, arg = tiling
    length = int(length)
    if length < 1:
        raise ValueError(f"gdl: a clip of {length} samples cannot be tiled")
    if kind == "times":
        return length * int(arg)
    if kind == "double":
        while length < int(arg):
            length *= 2
        return length
    raise ValueError(f"gdl: unknown tiling rule {tiling!r}")


def random_wave_starts(n, high, generator=None):
    """n window starts, each uniform in [0, high] with `high` included, like the datasets' random.randint(0, high); int64 [n] on
    the host.  One torch.randint call on `generator` (torch's global RNG if None): the distribution is the reference's, the stream
    of Python's Mersenne Twister that random.randint reads is not reproduced.  high = 0 draws nothing."""
    if high < 0:
        raise ValueError(f"gdl: the largest start {high} must not be negative")
    if high == 0:
        return torch.zeros(n, dtype=torch.int64)
    return torch.randint(0, int(high) + 1, (n,), generator=generator, dtype=torch.int64)


def wave_descriptors(clips_meta, starts, limits, n_samples):
    """The host half of wave_log_spectrogram: checks the windows and lays the clips out in one packed buffer.  clips_meta:
    [(len, channels, format)] with len in samples per channel and format GDL_WAVE_F32 / GDL_WAVE_S16 (or torch.float32 /
    torch.int16); starts, limits: one integer per clip.  Returns (desc, nbytes): the int64 [B, 6] table gdl_wave_logspec reads
    (byte offset, len, channels, format, start, limit) and the length of the packed buffer, every clip starting on a dword.
    Raises ValueError for len < 1, channels other than 1 or 2, an unknown format, a start below 0 and a window that ends past
    the tiled length, start + n_samples > limit: the reference would cut a shorter window there and yield a spectrogram of
    another shape, which its DataLoader cannot batch."""
    n_samples = int(n_samples)
    starts = torch.as_tensor(starts, dtype=torch.int64, device="cpu").reshape(-1).tolist()
    limits = torch.as_tensor(limits, dtype=torch.int64, device="cpu").reshape(-1).tolist()
    if len(clips_meta) == 0 or len(starts) != len(clips_meta) or len(limits) != len(clips_meta):
        raise ValueError(f"gdl: {len(clips_meta)} clips need as many starts and limits, not {len(starts)} and {len(limits)}")
    if n_samples < 1:
        raise ValueError(f"gdl: a window of {n_samples} samples")
    rows, offset = [], 0
    for i, ((length, channels, fmt), start, limit) in enumerate(zip(clips_meta, starts, limits)):
        fmt = _WAVE_FORMATS.get(fmt, fmt)
        length, channels = int(length), int(channels)
        if fmt not in _WAVE_BYTES:
            raise ValueError(f"gdl: clip {i} has format {fmt!r}; GDL_WAVE_F32 (float32) or GDL_WAVE_S16 (int16)")
        if length < 1 or length >= 1 << 31:
            raise ValueError(f"gdl: clip {i} has {length} samples")
        if channels not in (1, 2):
            raise ValueError(f"gdl: clip {i} has {channels} channels; one or two")
        if start < 0:
            raise ValueError(f"gdl: clip {i} starts its window at {start}")
        if start + n_samples > limit or limit >= 1 << 31:
            raise ValueError(f"gdl: the window [{start}, {start + n_samples}) of clip {i} does not lie inside its tiled length {limit} "
                             "(< 2^31): the reference would yield a shorter spectrogram here")
        rows.append([offset, length, channels, fmt, start, limit])
        offset += (length * channels * _WAVE_BYTES[fmt] + 3) // 4 * 4
    return torch.tensor(rows, dtype=torch.int64), offset


def _is_packed(clips):
    return isinstance(clips, tuple) and len(clips) == 2 and isinstance(clips[1], torch.Tensor) and clips[1].dtype == torch.int64


def _clip_meta(c):
    if not isinstance(c, torch.Tensor) or not c.is_cuda or c.dtype not in _WAVE_FORMATS or c.dim() not in (1, 2):
        raise ValueError("gdl: clips must be int16 or float32 device tensors [len] or [len, channels], or a (packed, desc) pair")
    return (int(c.shape[0]), 1 if c.dim() == 1 else int(c.shape[1]), _WAVE_FORMATS[c.dtype])


def pack_clips(clips):
    """A list of clips as one packed device buffer: (packed uint8 tensor, [(len, channels, format)]).  Every clip starts on a
    dword, at the offsets wave_descriptors gives.  A dataset that lives on the device does this once and then passes
    (packed, desc) to wave_log_spectrogram / stage_audio."""
    clips = list(clips)
    meta = [_clip_meta(c) for c in clips]
    parts = []
    for c in clips:
        raw = c.contiguous().reshape(-1).view(torch.uint8)
        parts.append(raw)
        if raw.numel() % 4:
            parts.append(torch.zeros(4 - raw.numel() % 4, dtype=torch.uint8, device=c.device))
    return torch.cat(parts), meta  # (a fresh allocation is aligned)


def wave_log_spectrogram(clips, n_samples, starts, limits, n_fft, hop_length, pad_mode="constant", resize=None, return_wave=False,
                         out=None):
    """From decoded clips to the datasets' log spectrograms in one launch: sample p of clip b's window is
    clip(mono_b[(starts[b] + p) mod len_b], -1, 1) for 0 <= p < n_samples -- the reference's np.tile(...)[start:start + n_samples]
    for either tiling rule, as long as starts[b] + n_samples <= limits[b], the tiled length -- with mono = x / 32768 for int16
    and the mean of the channels for stereo (librosa.load); then log_spectrogram of that window, bit for bit; then
    np.resize(spec, resize) if `resize` is given (a flat re-layout: the spectrogram's elements repeated or cut off in row-major
    order).

    clips: a list of device tensors, each int16 or float32 and [len] or [len, channels] with one or two channels (they are
    concatenated into one packed buffer), or a (packed, desc) pair for a dataset that already lives on the device: `packed` any
    contiguous device tensor holding the clips at the byte offsets of `desc`, the int64 [B, 6] table of wave_descriptors.  With
    the pair nothing is concatenated; starts / limits replace the table's columns where given (one small upload), and with both
    None a table that is on the device is used as it is.
    Resampling is not part of this: a clip is at its dataset's rate.  The 16 kHz datasets' wavs are stored at 16 kHz as 16-bit
    PCM and go in as int16; clips of the 22050 Hz datasets (CREMA-D, AVE) are resampled on the host and go in as float32.
    Returns float32 [B, n_fft//2+1, 1 + n_samples//hop_length], or [B, *resize]; with return_wave=True a pair of that and the
    staged windows, float32 [B, n_samples]."""
    if pad_mode not in PAD_MODES:
        raise ValueError(f"gdl: pad_mode must be one of {sorted(PAD_MODES)}, not {pad_mode!r}")
    n_samples = int(n_samples)
    if _is_packed(clips):
        packed, desc = clips
        if not isinstance(packed, torch.Tensor) or not packed.is_cuda or not packed.is_contiguous():
            raise ValueError("gdl: packed must be a contiguous device tensor")
        if desc.dim() != 2 or desc.shape[1] != 6 or desc.shape[0] < 1:
            raise ValueError("gdl: desc must be the int64 [B, 6] table of wave_descriptors")
        dev = packed.device
        if starts is not None or limits is not None or not desc.is_cuda:
            host = desc.cpu()
            starts = host[:, 4] if starts is None else starts
            limits = host[:, 5] if limits is None else limits
            checked, _ = wave_descriptors([tuple(r) for r in host[:, 1:4].tolist()], starts, limits, n_samples)
            checked[:, 0] = host[:, 0]
            desc = checked
        desc = desc.to(dev).contiguous()
    else:
        clips = list(clips)
        if not clips:
            raise ValueError("gdl: no clips")
        packed, meta = pack_clips(clips)
        dev = packed.device
        desc, nbytes = wave_descriptors(meta, starts, limits, n_samples)
        assert packed.numel() == nbytes
        desc = desc.to(dev)
    B = desc.shape[0]
    frames = L.load().gdl_logspec_frames(n_samples, hop_length)
    rh, rw = (0, 0) if resize is None else _size2(resize)
    shape = (B, n_fft // 2 + 1, frames) if resize is None else (B, rh, rw)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"gdl: out must be a contiguous float32 device tensor {list(shape)}")
    wave = torch.empty(B, n_samples, dtype=torch.float32, device=dev) if return_wave else None
    L.call("gdl_wave_logspec", L.ptr(packed), packed.numel() * packed.element_size(), L.ptr(desc), B, n_samples, n_fft, hop_length,
           PAD_MODES[pad_mode], rh, rw, L.ptr(wave), L.ptr(out), L.cur_stream())
    return (out, wave) if return_wave else out


def stage_audio(clips, dataset, starts=None, generator=None, pad_mode="constant", return_wave=False, out=None):
    """The audio half of a reference dataset's __getitem__ by name (AUDIO_STAGES), for a batch: tiled length by the dataset's
    rule, a window start per clip -- `starts`, or drawn by random_wave_starts from `generator` (torch's global RNG if None) in
    the dataset's range -- the window, the dataset's STFT and its np.resize.  The reference draws the window in test mode as well,
    so there is no train flag.  The draws have the reference's distribution; the stream of Python's Mersenne Twister behind its
    random.randint is not reproduced.  clips, the rest and the result as wave_log_spectrogram; the clips are at the dataset's
    rate (AUDIO_STAGES[dataset]["rate"]): nothing is resampled here, and the 22050 Hz datasets pass float32 clips that the host
    has resampled."""
    if dataset not in AUDIO_STAGES:
        raise ValueError(f"gdl: no audio stage for dataset {dataset!r}; one of {sorted(AUDIO_STAGES)}")
    st = AUDIO_STAGES[dataset]
    if _is_packed(clips):
        if not isinstance(clips[0], torch.Tensor) or not clips[0].is_cuda:
            raise ValueError("gdl: packed must be a contiguous device tensor")
        lengths = clips[1][:, 1].cpu().tolist()
    else:
        clips = list(clips)
        lengths = [_clip_meta(c)[0] for c in clips]
    limits = [wave_limit(n, st["tiling"]) for n in lengths]
    if starts is None:
        starts = random_wave_starts(len(lengths), st["start_high"], generator)
    return wave_log_spectrogram(clips, st["n_samples"], starts, limits, st["n_fft"], st["hop_length"], pad_mode, st["resize"],
                                return_wave, out)


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
