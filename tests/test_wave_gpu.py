"""gdl_wave_logspec / gdl.data.wave_log_spectrogram / stage_audio on the GPU: PCM decode, mono mix-down, tiling, window, clip,
log-magnitude STFT and np.resize in one launch.  The staged window is held bit for bit to the literal NumPy restatement
tests/wave_ref.py (the decode scale and the two-channel mean are exact or single fp32 operations, everything else selects
samples), the spectrogram bit for bit to gdl_logspec of that window (the two kernels share the transform's device code) and, with
the bounds of test_step_gpu.py's _check_logspec, to the float64 oracle; np.resize is a re-layout and is bit-exact too."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wave_ref as wr  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gdl import data as gd  # noqa: E402
from gpu_util import DEV  # noqa: E402

N_FFT, HOP, N = 64, 16, 1000  # the toy transform: 33 bins x 63 frames
PADS = ("constant", "reflect")


def _check_logspec(got, want):
    """The project's bounds for an fp32 direct DFT against a float64 transform (tests/test_step_gpu.py): the magnitudes agree to
    2e-5 of the largest one, the log values to 1e-3 wherever |X| >= 1e-2."""
    mg, mw = np.exp(got.astype(np.float64)) - 1e-7, np.exp(want.astype(np.float64)) - 1e-7
    assert np.abs(mg - mw).max() <= 2e-5 * max(1.0, mw.max())
    big = mw >= 1e-2
    np.testing.assert_allclose(got[big], want[big], rtol=0, atol=1e-3)


def _make_clip(rng, length, channels, dtype):
    shape = (length,) if channels == 1 else (length, 2)
    if dtype == np.int16:
        raw = rng.integers(-32768, 32768, shape).astype(np.int16)
        flat = raw.reshape(-1)  # both ends of the range, in both channels, and on both sides of a stereo pair
        vals = [-32768, 32767, 32767, 32767, -32768, -32768, 32767, -32768]
        flat[: min(len(vals), flat.size)] = vals[: flat.size]
        return raw
    raw = (rng.standard_normal(shape) * 0.7).astype(np.float32)
    raw.reshape(-1)[:: 5] *= 4.0  # well beyond +-1, before and after the mix-down
    return raw


def _toy_batch():
    """Every length x every start x every format: 72 clips.  limit: whole copies of the clip, enough for a window that starts at
    the clip's last sample, and one more, so that the largest start lies a period further on."""
    rng = np.random.default_rng(5)
    clips, starts, limits = [], [], []
    for length in (1, 7, 999, 1000, 1001, 2500):
        reps = -(-(length - 1 + N) // length) + 1
        limit = reps * length
        for start in (0, length - 1, limit - N):
            for channels, dtype in ((2, np.int16), (1, np.int16), (2, np.float32), (1, np.float32)):
                clips.append(_make_clip(rng, length, channels, dtype))
                starts.append(start)
                limits.append(limit)
    return clips, starts, limits


def _stage_all(clips, starts, limits, n):
    return np.stack([wr.stage(c, s, n, ("times", lim // len(c))) for c, s, lim in zip(clips, starts, limits)])


@pytest.fixture(scope="module")
def toy():
    """The toy batch through the kernel once per pad mode, and its restatement; shared and left unchanged."""
    clips, starts, limits = _toy_batch()
    dev_clips = [torch.from_numpy(c).to(DEV) for c in clips]
    staged = _stage_all(clips, starts, limits, N)
    got = {}
    for pad in PADS:
        spec, wave = gd.wave_log_spectrogram(dev_clips, N, starts, limits, N_FFT, HOP, pad, return_wave=True)
        got[pad] = (spec.cpu().numpy(), wave.cpu().numpy())
    return dict(clips=clips, dev_clips=dev_clips, starts=starts, limits=limits, staged=staged, got=got)


def test_staging_bit_exact(toy):
    assert toy["staged"].shape == (72, N) and np.abs(toy["staged"]).max() == 1.0
    for pad in PADS:
        wave = toy["got"][pad][1]
        assert wave.dtype == np.float32 and wave.shape == (72, N)
        np.testing.assert_array_equal(wave, toy["staged"])


@pytest.mark.parametrize("pad", PADS)
def test_spectrogram_bit_exact_against_logspec(toy, pad):
    want = gd.log_spectrogram(torch.from_numpy(toy["staged"]).to(DEV), N_FFT, HOP, pad).cpu().numpy()
    got = toy["got"][pad][0]
    assert got.shape == (72, N_FFT // 2 + 1, 1 + N // HOP) == want.shape
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("pad", PADS)
def test_spectrogram_against_restatement(toy, pad):
    _check_logspec(toy["got"][pad][0], wr.log_spectrogram(toy["staged"], N_FFT, HOP, pad))


@pytest.mark.parametrize("size", [(40, 40), (50, 50), (80, 80)], ids=["truncate", "one_wrap", "three_copies"])
def test_resize_bit_exact(toy, size):
    """33 x 63 = 2079 elements into 1600 (cut off), 2500 (421 written twice) and 6400 (three copies and 163 more)."""
    spec = toy["got"]["constant"][0]
    want = np.stack([np.resize(s, size) for s in spec])
    got, wave = gd.wave_log_spectrogram(toy["dev_clips"], N, toy["starts"], toy["limits"], N_FFT, HOP, resize=size, return_wave=True)
    assert tuple(got.shape) == (72,) + size
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(wave.cpu().numpy(), toy["staged"])
    out = torch.empty(72, *size, device=DEV)
    assert gd.wave_log_spectrogram(toy["dev_clips"], N, toy["starts"], toy["limits"], N_FFT, HOP, resize=size, out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy(), want)


REAL = {  # dataset: (clips as (length, channels, dtype), starts, output shape)
    "CREMAD_swin": ([(28665, 1, np.float32), (50001, 1, np.float32)], None, (224, 224)),          # 48316 elements wrap into 50176
    "AVE": ([(22050, 1, np.float32), (110250, 2, np.float32)], None, (224, 224)),                 # 66563 cut to 50176
    "KineticSound": ([(160000, 2, np.int16), (70001, 2, np.int16)], [80000, 33333], (129, 626)),
    "kinect400": ([(159999, 1, np.int16), (20000, 2, np.int16)], [32000, 1], (129, 1001)),
}


@pytest.mark.parametrize("name", list(REAL))
def test_real_shapes(name):
    metas, starts, shape = REAL[name]
    st = gd.AUDIO_STAGES[name]
    rng = np.random.default_rng(len(name))
    clips = [_make_clip(rng, *m) for m in metas]
    starts = [0] * len(clips) if starts is None else starts
    staged = np.stack([wr.stage(c, s, st["n_samples"], st["tiling"]) for c, s in zip(clips, starts)])
    got, wave = gd.stage_audio([torch.from_numpy(c).to(DEV) for c in clips], name, starts=starts, return_wave=True)
    assert tuple(got.shape) == (2,) + shape
    np.testing.assert_array_equal(wave.cpu().numpy(), staged)
    plain = gd.log_spectrogram(torch.from_numpy(staged).to(DEV), st["n_fft"], st["hop_length"]).cpu().numpy()
    want = plain if st["resize"] is None else np.stack([np.resize(s, st["resize"]) for s in plain])
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    _check_logspec(got.cpu().numpy(), wr.log_spectrogram(staged, st["n_fft"], st["hop_length"], resize=st["resize"]))


def test_by_name_seeded_and_packed():
    """stage_audio draws the starts from the generator: the same seed gives the same batch, and the batch is what
    wave_log_spectrogram gives for those starts.  The (packed, desc) form of a dataset that lives on the device gives it too."""
    rng = np.random.default_rng(11)
    clips = [torch.from_numpy(_make_clip(rng, *m)).to(DEV) for m in ((160000, 2, np.int16), (9999, 1, np.int16), (200001, 1, np.float32))]
    st = gd.AUDIO_STAGES["VGGSound"]
    a = gd.stage_audio(clips, "VGGSound", generator=torch.Generator().manual_seed(4))
    b, wave = gd.stage_audio(clips, "VGGSound", generator=torch.Generator().manual_seed(4), return_wave=True)
    assert torch.equal(a, b) and tuple(a.shape) == (3, 129, 626)
    starts = gd.random_wave_starts(3, st["start_high"], torch.Generator().manual_seed(4))
    assert len(set(starts.tolist())) == 3 and 0 <= min(starts.tolist()) and max(starts.tolist()) <= 80000
    limits = [gd.wave_limit(c.shape[0], st["tiling"]) for c in clips]
    assert limits == [160000, 319968, 200001]
    c = gd.wave_log_spectrogram(clips, st["n_samples"], starts, limits, st["n_fft"], st["hop_length"])
    assert torch.equal(a, c)
    other = gd.stage_audio(clips, "VGGSound", generator=torch.Generator().manual_seed(5))
    assert not torch.equal(a, other)
    # the dataset packed once; per step a table of starts
    packed, meta = gd.pack_clips(clips)
    desc, nbytes = gd.wave_descriptors(meta, [0, 0, 0], limits, st["n_samples"])
    assert packed.numel() == nbytes
    d = gd.stage_audio((packed, desc), "VGGSound", generator=torch.Generator().manual_seed(4))
    assert torch.equal(a, d)
    full, _ = gd.wave_descriptors(meta, starts, limits, st["n_samples"])
    e = gd.wave_log_spectrogram((packed, full.to(DEV)), st["n_samples"], None, None, st["n_fft"], st["hop_length"])  # the table as it is
    assert torch.equal(a, e)
    with pytest.raises(ValueError):  # the pair's windows are checked like the list's
        gd.wave_log_spectrogram((packed, desc), st["n_samples"], [0, 0, 200001], None, st["n_fft"], st["hop_length"])


def _call_abi(packed, rows, n, resize=(0, 0)):
    desc = torch.tensor(rows, dtype=torch.int64).to(DEV)
    B = len(rows)
    frames = 1 + n // HOP
    shape = (B, N_FFT // 2 + 1, frames) if resize == (0, 0) else (B,) + resize
    out = torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    wave = torch.full((B, n), 7.0, dtype=torch.float32, device=DEV)
    L.call("gdl_wave_logspec", L.ptr(packed), packed.numel(), L.ptr(desc), B, n, N_FFT, HOP, 0, resize[0], resize[1], L.ptr(wave),
           L.ptr(out), L.cur_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), wave.cpu().numpy()


def test_bad_sample_is_nan_and_never_read():
    """One sample of three has a descriptor that the kernel must refuse -- a clip that lies past the end of the packed buffer
    first of all: its rows are NaN in both outputs, its neighbours are bit-equal to the good run.  The guard comes before
    any read, so nothing out of bounds is touched."""
    rng = np.random.default_rng(2)
    clips = [torch.from_numpy(_make_clip(rng, *m)).to(DEV) for m in ((700, 2, np.int16), (1500, 1, np.float32), (333, 1, np.int16))]
    packed, meta = gd.pack_clips(clips)
    desc, nbytes = gd.wave_descriptors(meta, [5, 100, 0], [7000, 3000, 3330], N)
    good = desc.tolist()
    want_spec, want_wave = _call_abi(packed, good, N)
    assert np.isfinite(want_spec).all() and np.isfinite(want_wave).all()
    off, length = good[1][0], good[1][1]
    bad_rows = {
        "past the end": [nbytes - 8, length, 1, 0, 100, 3000],
        "offset beyond the buffer": [nbytes + 4096, length, 1, 0, 100, 3000],
        "longer than the buffer": [off, (nbytes - off) // 4 + 1, 1, 0, 100, 3000],
        "two channels do not fit": [off, (nbytes - off) // 8 + 1, 2, 0, 100, 3000],
        "huge length": [off, 1 << 40, 1, 0, 100, 3000],
        "negative offset": [-4, length, 1, 0, 100, 3000],
        "offset off the dword": [off + 2, length - 1, 1, 0, 100, 3000],
        "no samples": [off, 0, 1, 0, 100, 3000],
        "three channels": [off, 10, 3, 0, 100, 3000],
        "no channels": [off, 10, 0, 0, 100, 3000],
        "unknown format": [off, 10, 1, 2, 100, 3000],
        "negative start": [off, length, 1, 0, -1, 3000],
        "window past the limit": [off, length, 1, 0, 2001, 3000],
        "limit of 2^31": [off, length, 1, 0, 100, 1 << 31],
        "start that overflows": [off, length, 1, 0, (1 << 63) - 1, 3000],
    }
    for what, row in bad_rows.items():
        for resize in ((0, 0), (50, 50)):
            spec, wave = _call_abi(packed, [good[0], row, good[2]], N, resize)
            assert np.isnan(spec[1]).all() and np.isnan(wave[1]).all(), what
            np.testing.assert_array_equal(wave[[0, 2]], want_wave[[0, 2]], err_msg=what)
            if resize == (0, 0):
                np.testing.assert_array_equal(spec[[0, 2]], want_spec[[0, 2]], err_msg=what)
            else:
                np.testing.assert_array_equal(spec[[0, 2]], np.stack([np.resize(s, resize) for s in want_spec[[0, 2]]]), err_msg=what)


def test_arguments():
    clip = torch.zeros(2000, dtype=torch.int16, device=DEV)
    for fn in (lambda: gd.wave_log_spectrogram([clip], N, [0], [2000], N_FFT, HOP, pad_mode="edge"),
               lambda: gd.wave_log_spectrogram([clip.to(torch.int32)], N, [0], [2000], N_FFT, HOP),
               lambda: gd.wave_log_spectrogram([clip.reshape(-1, 4)], N, [0], [2000], N_FFT, HOP),       # four channels
               lambda: gd.wave_log_spectrogram([clip], N, [1001], [2000], N_FFT, HOP),                  # window past the limit
               lambda: gd.wave_log_spectrogram([clip], N, [0], [2000], N_FFT, HOP, resize=(0, 5)),
               lambda: gd.wave_log_spectrogram([clip], N, [0], [2000], N_FFT, HOP, out=torch.empty(1, 33, 62, device=DEV)),
               lambda: gd.wave_log_spectrogram([], N, [], [], N_FFT, HOP)):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(L.GdlError):
        gd.wave_log_spectrogram([clip], N, [0], [2000], 48, HOP)  # not a power of two
    with pytest.raises(L.GdlError):
        gd.wave_log_spectrogram([clip], 20, [0], [2000], N_FFT, HOP, pad_mode="reflect")
    silent = gd.wave_log_spectrogram([clip], N, [0], [2000], N_FFT, HOP)
    np.testing.assert_allclose(silent.cpu().numpy(), np.log(np.float32(1e-7)), rtol=0, atol=1e-5)
