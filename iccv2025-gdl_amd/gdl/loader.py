"""The device-resident epoch loader over gdl_loader_plan / gdl_wave_logspec / gdl_frames_resized_crop.

gdl.data stages a batch on the device but draws its window starts, crop boxes and flips in Python and uploads two tables per
batch.  Here the decoded dataset lives on the device (DeviceDataset: the clips and the first T frames of every sample, packed
once), and the shuffle, the draws and the descriptor tables are a function of (seed, epoch, sample) computed there:

    ds = gdl.DeviceDataset(clips, frames, labels, "KineticSound", T=3)
    loader = gdl.DeviceLoader(ds, batch_size=64, train=True, seed=0)
    for epoch in range(epochs):
        loader.set_epoch(epoch)
        for spec, image, label in loader:      # one planning launch per epoch, two staging launches per batch
            trainer.step(spec, image, label)   # no host random numbers, no host-to-device copy, no synchronisation

The draws are Philox words keyed by the sample's index (include/gdl_hip.h, gdl_loader_plan): they have the reference's
distributions, not its random streams, as gdl.data's.  Nothing is computed on the CPU and there is no fallback.
"""
import ctypes
import math

import torch

from . import _lib as L
from . import data as D

_STAGE_KEYS = ("n_samples", "tiling", "start_high", "n_fft", "hop_length", "resize")


def _audio_stage(audio):
    if isinstance(audio, str):
        if audio not in D.AUDIO_STAGES:
            raise ValueError(f"gdl: no audio stage for dataset {audio!r}; one of {sorted(D.AUDIO_STAGES)}")
        audio = D.AUDIO_STAGES[audio]
    if not isinstance(audio, dict) or any(k not in audio for k in _STAGE_KEYS):
        raise ValueError(f"gdl: audio must be a name in AUDIO_STAGES or a dict with the keys {list(_STAGE_KEYS)}")
    st = {k: audio[k] for k in _STAGE_KEYS}
    st["n_samples"], st["start_high"] = int(st["n_samples"]), int(st["start_high"])
    st["n_fft"], st["hop_length"] = int(st["n_fft"]), int(st["hop_length"])
    if st["n_samples"] < 1 or st["start_high"] < 0:
        raise ValueError(f"gdl: a window of {st['n_samples']} samples starting at up to {st['start_high']}")
    return st


def _device(device, hint=None):
    if device is None:
        device = hint if hint is not None and hint.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"gdl: a DeviceDataset lives on a GPU, not on {device}; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


class DeviceDataset:
    """A decoded audio-visual dataset on the device: every clip and the first T frames of every sample in two packed buffers,
    with the three int64 tables gdl_loader_plan reads -- clips [N, 5] (byte offset, len, channels, format, tiled length), frames
    [N, T, 3] (byte offset, H, W) and labels [N].

    clips: N int16 / float32 tensors [len] or [len, channels] (one or two channels), on the host or the device, at the dataset's
    rate (gdl.data.stage_audio).  frames: N sequences of T uint8 [H, W, 3] tensors, or one uint8 [N, T, H, W, 3] tensor: the
    first T frames of each sample, which is what the reference's datasets read.  labels: N integers.  audio: a name in
    gdl.data.AUDIO_STAGES or a dict with its keys (n_samples, tiling, start_high, n_fft, hop_length, resize).  size: the
    images' output size, int or (height, width).

    Checked once, on the host, naming the offending sample: every window the planner can draw ends inside its clip's tiled
    length (start_high + n_samples <= limit), the whole frame of every distinct frame size fits the resize kernel
    (gdl_frames_resized_crop_box_ok; every box inside it then does), the labels are integers."""

    def __init__(self, clips, frames, labels, audio, T, size=224, device=None):
        clips = list(clips)
        T = int(T)
        if not clips:
            raise ValueError("gdl: an empty dataset")
        if T < 1 or T > 64:
            raise ValueError(f"gdl: T = {T} frames per sample; 1 to 64")
        for i, c in enumerate(clips):
            if not isinstance(c, torch.Tensor) or c.dtype not in (torch.int16, torch.float32) or c.dim() not in (1, 2):
                raise ValueError(f"gdl: clip {i} must be an int16 or float32 tensor [len] or [len, channels]")
        dev = _device(device, clips[0].device)
        N = len(clips)
        if isinstance(frames, torch.Tensor):
            if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 or frames.shape[0] != N or frames.shape[1] != T:
                raise ValueError(f"gdl: frames must be a uint8 tensor [{N}, {T}, H, W, 3] or {N} sequences of {T} uint8 [H, W, 3] tensors")
            flat = list(frames.reshape(N * T, *frames.shape[2:]).unbind(0))
        else:
            frames = [list(f.unbind(0)) if isinstance(f, torch.Tensor) and f.dim() == 4 else list(f) for f in frames]
            if len(frames) != N:
                raise ValueError(f"gdl: {N} clips but frames of {len(frames)} samples")
            for i, fs in enumerate(frames):
                if len(fs) != T:
                    raise ValueError(f"gdl: sample {i} has {len(fs)} frames, not T = {T}")
                for f in fs:
                    if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3:
                        raise ValueError(f"gdl: the frames of sample {i} must be uint8 tensors [H, W, 3]")
            flat = [f for fs in frames for f in fs]
        labels = torch.as_tensor(labels)
        if labels.dim() != 1 or labels.shape[0] != N or labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
            raise ValueError(f"gdl: labels must be {N} integers, not {labels.dtype} {list(labels.shape)}")

        wave, meta = D.pack_clips([c.to(dev) for c in clips])
        tiling = _audio_stage(audio)["tiling"]
        rows, offset = [], 0
        for length, channels, fmt in meta:
            rows.append([offset, length, channels, fmt, D.wave_limit(length, tiling)])
            offset += (length * channels * D._WAVE_BYTES[fmt] + 3) // 4 * 4
        assert offset == wave.numel()
        if isinstance(frames, torch.Tensor) and (frames.shape[2] * frames.shape[3] * 3) % 4 == 0:
            h, w = int(frames.shape[2]), int(frames.shape[3])  # one size, every frame on a dword as it stands: no copy on the device
            pixels = frames.to(dev).contiguous().reshape(-1)
            ftab = torch.tensor([h * w * 3, 0, 0]) * torch.arange(N * T).reshape(-1, 1) + torch.tensor([0, h, w])
        else:
            frows, offset, parts = [], 0, []
            for f in flat:
                h, w = int(f.shape[0]), int(f.shape[1])
                frows.append([offset, h, w])
                parts.append(f.to(dev).reshape(-1))
                pad = -(h * w * 3) % 4
                if pad:
                    parts.append(torch.zeros(pad, dtype=torch.uint8, device=dev))
                offset += h * w * 3 + pad
            pixels, ftab = torch.cat(parts), torch.tensor(frows, dtype=torch.int64)
        self._init(wave, torch.tensor(rows, dtype=torch.int64), pixels, ftab.reshape(N, T, 3), labels.to(torch.int64), audio, T, size)

    @classmethod
    def from_packed(cls, wave, clips, pixels, frames, labels, audio, T, size=224):
        """For a caller who already holds the packed buffers and the tables: wave / pixels are contiguous device tensors (any
        dtype; 4-byte aligned, every clip and frame starting on a dword, as gdl.data.pack_clips / crop_descriptors lay them
        out), clips int64 [N, 5], frames int64 [N, T, 3], labels int64 [N], on the host or the device.  The same checks run
        (the tables are read back once if they are on the device)."""
        self = cls.__new__(cls)
        for name, t in (("wave", wave), ("pixels", pixels)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or t.data_ptr() % 4:
                raise ValueError(f"gdl: {name} must be a contiguous, 4-byte aligned device tensor; a DeviceDataset lives on a GPU")
        if pixels.device != wave.device:
            raise ValueError("gdl: wave and pixels must be on one device")
        for name, t in (("clips", clips), ("frames", frames), ("labels", labels)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
                raise ValueError(f"gdl: {name} must be an int64 tensor")
        self._init(wave, clips.cpu(), pixels, frames.cpu(), labels.cpu(), audio, int(T), size)
        return self

    def _init(self, wave, clips, pixels, frames, labels, audio, T, size):
        st = _audio_stage(audio)
        out_h, out_w = D._size2(size)
        N = int(labels.shape[0])
        if T < 1 or T > 64:
            raise ValueError(f"gdl: T = {T} frames per sample; 1 to 64")
        if N < 1 or N >= 1 << 31 or labels.dim() != 1 or tuple(clips.shape) != (N, 5) or tuple(frames.shape) != (N, T, 3):
            raise ValueError(f"gdl: tables of {N} samples must be clips [{N}, 5], frames [{N}, {T}, 3], labels [{N}], not "
                             f"{list(clips.shape)}, {list(frames.shape)}, {list(labels.shape)}")
        wave_bytes, pixel_bytes = wave.numel() * wave.element_size(), pixels.numel() * pixels.element_size()
        lib = L.load()
        if not lib.gdl_frames_resized_crop_box_ok(1, 1, out_h, out_w):
            raise ValueError(f"gdl: output size {out_h} x {out_w} does not fit the resize kernel's tables")
        need = st["start_high"] + st["n_samples"]
        for i, (off, length, channels, fmt, limit) in enumerate(clips.tolist()):
            if fmt not in D._WAVE_BYTES or channels not in (1, 2) or length < 1 or length >= 1 << 31:
                raise ValueError(f"gdl: clip {i} has {length} samples of {channels} channels in format {fmt}")
            if off < 0 or off % 4 or off + length * channels * D._WAVE_BYTES[fmt] > wave_bytes:
                raise ValueError(f"gdl: clip {i} at byte {off} does not lie on a dword inside the packed buffer of {wave_bytes} bytes")
            if need > limit or limit >= 1 << 31:
                raise ValueError(f"gdl: clip {i}: a window of {st['n_samples']} samples starting at up to {st['start_high']} does not "
                                 f"lie inside its tiled length {limit} (< 2^31): the reference would yield a shorter spectrogram here")
        sizes = {}
        for i, per_sample in enumerate(frames.tolist()):
            for off, h, w in per_sample:
                if h < 1 or w < 1 or h > 65535 or w > 65535 or off < 0 or off % 4 or off + h * w * 3 > pixel_bytes:
                    raise ValueError(f"gdl: a {h} x {w} frame of sample {i} at byte {off} does not lie on a dword inside the packed "
                                     f"buffer of {pixel_bytes} bytes")
                sizes.setdefault((h, w), i)
        for (h, w), i in sizes.items():
            if not lib.gdl_frames_resized_crop_box_ok(h, w, out_h, out_w):
                raise ValueError(f"gdl: the {h} x {w} frames (first in sample {i}) -> {out_h} x {out_w} do not fit the resize kernel's "
                                 "40 KB of LDS (include/gdl_hip.h, gdl_frames_resized_crop: limits)")
        dev = wave.device
        self.device, self.N, self.T, self.size, self.audio = dev, N, T, (out_h, out_w), st
        self.wave, self.pixels = wave, pixels
        self.wave_bytes, self.pixel_bytes = wave_bytes, pixel_bytes
        self.clips, self.frames, self.labels = clips.to(dev).contiguous(), frames.to(dev).contiguous(), labels.to(dev).contiguous()

    def __len__(self):
        return self.N

    @property
    def nbytes(self):
        """Device memory the dataset holds: the two packed buffers and the three tables."""
        return self.wave_bytes + self.pixel_bytes + 8 * (self.clips.numel() + self.frames.numel() + self.labels.numel())


class DeviceLoader:
    """An epoch of (spec, image, label) batches of a DeviceDataset, in the shapes and dtypes DGLTrainer.step / UnimodalTrainer.step
    / valid take: float32 [B, bins, frames] (or [B, *resize]), float32 [B, 3, T, h, w], int64 [B].

    train sets both the shuffle and the augmentation (RandomResizedCrop + RandomHorizontalFlip; otherwise file order and
    Resize); the window start is drawn in either mode, as the reference does.  len(loader) = N // (batch_size * world_size): the
    remainder is dropped, as both of the reference's DataLoaders do.  Rank r's batch k holds the epoch positions
    (k * world_size + r) * batch_size .. ; a sample's window, boxes and flips depend on (seed, epoch, sample) only, not on the
    batch size or the rank layout.  set_epoch(e) before iterating, as with a DistributedSampler.

    iter() makes one gdl_loader_plan launch for the epoch; next() makes the two stage launches into one of `depth` rotating
    output buffers and returns views: a batch is rewritten by the `depth`-th next() after its own (with stream=, where a batch
    is staged one call ahead, behind the work enqueued before the (depth - 1)-th); a caller who keeps batches longer clones
    them or raises depth.  No host copy and no synchronisation happens per batch.  iter() continues at the next batch of
    state_dict(); set_epoch() and the end of an epoch rewind to batch 0.
    stream: a torch.cuda.Stream on which batch k + 1 is staged while the caller works on batch k (depth >= 2): the current
    stream waits for a buffer's ready event at next(), and the side stream waits for the event recorded on the current stream at
    the following next() before it rewrites that buffer.  The bytes are the same with and without it; measured, it does not
    shorten the trainer loop (profiles/loader_bench.txt), so None is the default.
    plan() returns host copies of the epoch's four tables and is the only call that synchronises.  state_dict() /
    load_state_dict() hold (seed, epoch, next batch): a resumed loader continues with identical bytes."""

    def __init__(self, ds, batch_size, train, seed=0, rank=0, world_size=1, pad_mode="constant", scale=(0.08, 1.0),
                 ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip=0.5, depth=2, stream=None, mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD):
        if not isinstance(ds, DeviceDataset):
            raise ValueError("gdl: DeviceLoader reads a gdl.DeviceDataset (a dataset on the host has no loader here: there is no CPU path)")
        B, world_size, rank, depth = int(batch_size), int(world_size), int(rank), int(depth)
        if B < 1 or B > 65535:
            raise ValueError(f"gdl: batch_size {B}; 1 to 65535")
        if world_size < 1 or not 0 <= rank < world_size:
            raise ValueError(f"gdl: rank {rank} of world_size {world_size}")
        if B * world_size > ds.N:
            raise ValueError(f"gdl: batch_size * world_size = {B * world_size} exceeds the dataset's {ds.N} samples: no full batch")
        if depth < 1:
            raise ValueError(f"gdl: depth {depth}; at least one output buffer")
        if stream is not None:
            if not isinstance(stream, torch.cuda.Stream) or stream.device != ds.device:
                raise ValueError("gdl: stream must be a torch.cuda.Stream on the dataset's device")
            if depth < 2:
                raise ValueError("gdl: with stream= the next batch is staged while the caller still reads this one; depth = 1 would "
                                 "rewrite a buffer in use: depth must be at least 2")
        if pad_mode not in D.PAD_MODES:
            raise ValueError(f"gdl: pad_mode must be one of {sorted(D.PAD_MODES)}, not {pad_mode!r}")
        scale, ratio, p_flip = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1])), float(p_flip)
        if not (0 < scale[0] <= scale[1] and 0 < ratio[0] <= ratio[1] and 0 <= p_flip <= 1):
            raise ValueError(f"gdl: scale {scale}, ratio {ratio}, p_flip {p_flip}: positive ascending ranges and a probability")
        self.ds, self.batch_size, self.train, self.rank, self.world_size, self.depth, self.stream = ds, B, bool(train), rank, world_size, depth, stream
        self.seed, self.epoch, self._next = int(seed) & (1 << 64) - 1, 0, 0
        self.pad_mode = D.PAD_MODES[pad_mode]
        # the logarithms are taken here, so that the device and a restatement of it use the same constants
        self._draw = (ctypes.c_double * 7)(scale[0], scale[1], ratio[0], ratio[1], math.log(ratio[0]), math.log(ratio[1]), p_flip)
        self._mean = (ctypes.c_float * 3)(*[float(v) for v in mean])
        self._std = (ctypes.c_float * 3)(*[float(v) for v in std])
        self._len = ds.N // (B * world_size)
        P = self._len * world_size * B  # the epoch's positions, every rank's
        dev, st = ds.device, ds.audio
        self._index = torch.empty(P, dtype=torch.int64, device=dev)
        self._label = torch.empty(P, dtype=torch.int64, device=dev)
        self._wave_desc = torch.empty(P, 6, dtype=torch.int64, device=dev)
        self._crop_desc = torch.empty(P * ds.T, 8, dtype=torch.int64, device=dev)
        self._resize = (0, 0) if st["resize"] is None else D._size2(st["resize"])
        frames = L.load().gdl_logspec_frames(st["n_samples"], st["hop_length"])
        spec_shape = (B, st["n_fft"] // 2 + 1, frames) if st["resize"] is None else (B, *self._resize)
        self._spec = [torch.empty(spec_shape, dtype=torch.float32, device=dev) for _ in range(depth)]
        self._image = [torch.empty(B, 3, ds.T, *ds.size, dtype=torch.float32, device=dev) for _ in range(depth)]
        self._ready = [torch.cuda.Event() for _ in range(depth)] if stream is not None else None
        self._consumed = [torch.cuda.Event() for _ in range(depth)] if stream is not None else None
        self._planned = None   # (seed, epoch) the tables hold
        self._staged = None    # the batch the side stream has staged ahead
        self._yielded = None   # the buffer the caller holds

    def __len__(self):
        return self._len

    def set_epoch(self, epoch):
        self.epoch, self._next = int(epoch), 0

    def state_dict(self):
        return {"seed": self.seed, "epoch": self.epoch, "next_batch": self._next}

    def load_state_dict(self, state):
        nxt = int(state["next_batch"])
        if not 0 <= nxt <= self._len:
            raise ValueError(f"gdl: next_batch {nxt} of an epoch of {self._len} batches")
        self.seed, self.epoch, self._next = int(state["seed"]) & (1 << 64) - 1, int(state["epoch"]), nxt

    def _plan(self):
        """The epoch's planning launch on the current stream (skipped if the tables already hold this seed and epoch)."""
        if self._planned == (self.seed, self.epoch):
            return
        ds, st = self.ds, self.ds.audio
        L.call("gdl_loader_plan", L.ptr(ds.clips), L.ptr(ds.frames), L.ptr(ds.labels), ds.N, ds.T, self.seed, self.epoch, 0,
               self._index.numel(), int(self.train), int(self.train), st["n_samples"], st["start_high"], ds.size[0], ds.size[1],
               ctypes.cast(self._draw, ctypes.c_void_p), L.ptr(self._index), L.ptr(self._label), L.ptr(self._wave_desc),
               L.ptr(self._crop_desc), L.cur_stream())
        self._planned = (self.seed, self.epoch)

    def plan(self):
        """Host copies of the epoch's tables: dict(index [P], label [P], wave_desc [P, 6], crop_desc [P * T, 8]) for the P =
        len * world_size * batch_size positions of every rank.  The only call that synchronises."""
        with torch.cuda.device(self.ds.device):
            self._quiesce()
            self._plan()
            return dict(index=self._index.cpu(), label=self._label.cpu(), wave_desc=self._wave_desc.cpu(), crop_desc=self._crop_desc.cpu())

    def _quiesce(self):
        """Order the side stream and the current stream behind each other before the tables or a staged buffer are rewritten."""
        if self.stream is not None:
            cur = torch.cuda.current_stream(self.ds.device)
            cur.wait_stream(self.stream)
            self.stream.wait_stream(cur)
        self._staged = self._yielded = None

    def _stage(self, k, stream_handle):
        """The two stage launches of this rank's batch k into buffer k % depth."""
        ds, st, B = self.ds, self.ds.audio, self.batch_size
        pos, slot = (k * self.world_size + self.rank) * B, k % self.depth
        L.call("gdl_wave_logspec", L.ptr(ds.wave), ds.wave_bytes, self._wave_desc.data_ptr() + 48 * pos, B, st["n_samples"], st["n_fft"],
               st["hop_length"], self.pad_mode, self._resize[0], self._resize[1], None, L.ptr(self._spec[slot]), stream_handle)
        L.call("gdl_frames_resized_crop", L.ptr(ds.pixels), ds.pixel_bytes, self._crop_desc.data_ptr() + 64 * pos * ds.T, B * ds.T, B, ds.T,
               ds.size[0], ds.size[1], ctypes.cast(self._mean, ctypes.c_void_p), ctypes.cast(self._std, ctypes.c_void_p),
               L.ptr(self._image[slot]), stream_handle)

    def _stage_ahead(self, k):
        slot = k % self.depth
        self.stream.wait_event(self._consumed[slot])  # (an event never recorded is complete)
        self._stage(k, self.stream.cuda_stream)
        self._ready[slot].record(self.stream)
        self._staged = k

    def __iter__(self):
        with torch.cuda.device(self.ds.device):
            self._quiesce()
            self._plan()
            if self.stream is not None:
                self.stream.wait_stream(torch.cuda.current_stream(self.ds.device))  # behind the plan
                if self._next < self._len:
                    self._stage_ahead(self._next)
        return self

    def __next__(self):
        k = self._next
        if k >= self._len:
            self._next = 0
            raise StopIteration
        if self._planned != (self.seed, self.epoch):
            raise L.GdlError("DeviceLoader: next() before iter(): the epoch has not been planned")
        B, slot = self.batch_size, k % self.depth
        with torch.cuda.device(self.ds.device):
            if self.stream is None:
                self._stage(k, L.cur_stream())
            else:
                cur = torch.cuda.current_stream(self.ds.device)
                if self._yielded is not None:  # the caller's work on the previous batch is enqueued: its buffer may be rewritten behind it
                    self._consumed[self._yielded].record(cur)
                if self._staged != k:
                    self._stage_ahead(k)
                cur.wait_event(self._ready[slot])
                self._yielded = slot
                if k + 1 < self._len:
                    self._stage_ahead(k + 1)
        self._next = k + 1
        pos = (k * self.world_size + self.rank) * B
        return self._spec[slot], self._image[slot], self._label[pos:pos + B]
