"""NumPy restatement of what gdl.data.wave_log_spectrogram / gdl_wave_logspec (csrc/input.hip) computes, in the order the
reference's datasets do it on the host (dataset/KSDataset.py:139-149, CramedDataset.py:60-66 and the same lines of the others):

    librosa.load          16-bit PCM is read as x / 32768 in float32 (soundfile's float read); mono=True is np.mean over the
                          channels in float32
    tiling                np.tile(samples, 3)                      (CREMA-D, AVE), or
                          while len(sample) / rate < 10.: sample = np.tile(sample, 2)      (the 16 kHz datasets)
    window                sample[start:start + n]
    clip                  x[x > 1.] = 1.; x[x < -1.] = -1.
    log spectrogram       np.log(np.abs(librosa.stft(x, n_fft, hop_length)) + 1e-7): oracle.log_spectrogram, the project's float64
                          restatement of librosa's published algorithm
    np.resize             where the dataset has one

The tiling and the slicing are done literally here -- the kernel's (start + p) mod len is what is under test.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as orc  # noqa: E402


def decode(raw):
    """What librosa.load returns before any resampling: float32, int16 scaled by 1 / 32768."""
    raw = np.asarray(raw)
    if raw.dtype == np.int16:
        return raw.astype(np.float32) / np.float32(32768.0)
    assert raw.dtype == np.float32
    return raw


def mono(x):
    """mono=True: the mean over the channels of a [len, channels] clip, in float32."""
    return np.mean(x, axis=1, dtype=np.float32) if x.ndim == 2 else x


def tile(sample, tiling):
    """("times", k): np.tile(sample, k).  ("double", m): the datasets' doubling loop with rate = m / 10, so that it runs while the
    clip is shorter than m samples (m = 160000 at 16 kHz)."""
    kind, arg = tiling
    if kind == "times":
        return np.tile(sample, arg)
    assert kind == "double" and arg % 10 == 0
    rate = arg // 10
    while len(sample) / rate < 10.:
        sample = np.tile(sample, 2)
    return sample


def stage(raw, start, n, tiling):
    """One clip as the file holds it -> the clipped window float32 [n]."""
    sample = tile(mono(decode(raw)), tiling)
    new_sample = sample[start:start + n].copy()
    assert len(new_sample) == n, "the window must end inside the tiled clip"
    new_sample[new_sample > 1.] = 1.
    new_sample[new_sample < -1.] = -1.
    return new_sample


def stage_modulo(raw, start, n):
    """The same window as the periodic extension of the clip: staged[p] = mono[(start + p) mod len]."""
    m = mono(decode(raw))
    w = m[(start + np.arange(n)) % len(m)].copy()
    w[w > 1.] = 1.
    w[w < -1.] = -1.
    return w


def log_spectrogram(staged, n_fft, hop, pad_mode="constant", resize=None):
    """staged: float32 [B][n] -> float32 [B][bins][frames], or [B][*resize] under np.resize."""
    spec = orc.log_spectrogram(staged, n_fft, hop, pad_mode)
    return spec if resize is None else np.stack([np.resize(s, resize) for s in spec])
