"""CPU-only checks of the device-side waveform staging (gdl.data.wave_log_spectrogram / stage_audio / gdl_wave_logspec): the
descriptor table and the datasets' tiling rules, the identity the kernel rests on -- the reference's np.tile + slice is the
periodic extension of the clip -- checked on the literal restatement tests/wave_ref.py, the argument errors of the C entry point
(refused before anything is dereferenced or launched), and that nothing runs on a host tensor."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wave_ref as wr  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gdl import data as gd  # noqa: E402


def test_descriptors_offsets_and_dword_padding():
    """An int16 mono clip of 7 samples is 14 bytes: the next clip starts at 16.  An int16 stereo clip of 5 is 20 bytes, a
    float32 mono clip of 3 is 12, a float32 stereo clip of 2 is 16."""
    meta = [(7, 1, gd.GDL_WAVE_S16), (5, 2, torch.int16), (3, 1, gd.GDL_WAVE_F32), (2, 2, torch.float32), (1, 1, gd.GDL_WAVE_S16)]
    desc, nbytes = gd.wave_descriptors(meta, [0, 4, 2, 1, 0], [21, 15, 9, 6, 3], 3)
    assert desc.dtype == torch.int64 and tuple(desc.shape) == (5, 6)
    assert desc[:, 0].tolist() == [0, 16, 36, 48, 64] and nbytes == 68
    assert desc[:, 1:].tolist() == [[7, 1, 1, 0, 21], [5, 2, 1, 4, 15], [3, 1, 0, 2, 9], [2, 2, 0, 1, 6], [1, 1, 1, 0, 3]]
    assert all(o % 4 == 0 for o in desc[:, 0].tolist())
    assert (gd.GDL_WAVE_F32, gd.GDL_WAVE_S16) == (0, 1)  # include/gdl_hip.h
    header = open(os.path.join(ROOT, "include", "gdl_hip.h")).read()
    assert "#define GDL_WAVE_F32 0" in header and "#define GDL_WAVE_S16 1" in header


def test_audio_stages_table_and_limits():
    """AUDIO_STAGES is the reference datasets' audio settings; wave_limit their tiled lengths: three copies, or doubled until
    ten seconds at 16 kHz are reached."""
    want = {  # name: (rate, window, largest start, n_fft, hop, resize, spectrogram [bins, frames])
        "CREMAD": (22050, 66150, 0, 512, 353, None, (257, 188)),
        "CREMAD_swin": (22050, 66150, 0, 512, 353, (224, 224), (257, 188)),
        "AVE": (22050, 66150, 0, 512, 256, (224, 224), (257, 259)),
        "KineticSound": (16000, 80000, 80000, 256, 128, None, (129, 626)),
        "VGGSound": (16000, 80000, 80000, 256, 128, None, (129, 626)),
        "kinect400": (16000, 128000, 32000, 256, 128, None, (129, 1001)),
        "Audioset": (16000, 80000, 80000, 512, 256, (224, 224), (257, 313)),
    }
    assert set(gd.AUDIO_STAGES) == set(want)
    lib = L.load()
    for name, (rate, n, high, n_fft, hop, resize, shape) in want.items():
        st = gd.AUDIO_STAGES[name]
        assert (st["rate"], st["n_samples"], st["start_high"], st["n_fft"], st["hop_length"], st["resize"]) == (rate, n, high, n_fft, hop, resize)
        assert (n_fft // 2 + 1, lib.gdl_logspec_frames(n, hop)) == shape
        if rate == 22050:
            assert st["tiling"] == ("times", 3)
            assert [gd.wave_limit(v, st["tiling"]) for v in (1, 22050, 66150, 100000)] == [3, 66150, 198450, 300000]
        else:
            assert st["tiling"] == ("double", 160000)
            assert [gd.wave_limit(v, st["tiling"]) for v in (1, 79999, 80000, 80001, 159999, 160000, 160001, 500000)] == \
                [262144, 319996, 160000, 160002, 319998, 160000, 160001, 500000]
            # the largest start the dataset draws always fits: start_high + window <= 160000 <= the tiled length
            assert high + n <= 160000
    # the limits are the lengths of the literal tiling
    for v in (1, 7, 159, 160, 161, 400):
        assert gd.wave_limit(v, ("double", 160)) == len(wr.tile(np.zeros(v, np.float32), ("double", 160)))
        assert gd.wave_limit(v, ("times", 3)) == len(wr.tile(np.zeros(v, np.float32), ("times", 3)))
    with pytest.raises(ValueError):
        gd.wave_limit(0, ("times", 3))


def test_descriptor_errors():
    ok = [(10, 1, gd.GDL_WAVE_S16)]
    gd.wave_descriptors(ok, [20], [30], 10)  # start + n == limit: the last window that fits
    for meta, starts, limits, n in (([(0, 1, 0)], [0], [30], 10),        # len < 1
                                    ([(10, 0, 0)], [0], [30], 10),       # channels
                                    ([(10, 3, 1)], [0], [30], 10),
                                    ([(10, 1, 2)], [0], [30], 10),       # format
                                    (ok, [-1], [30], 10),                # start below 0
                                    (ok, [21], [30], 10),                # start + n > limit
                                    (ok, [0], [1 << 31], 10),            # a tiled length the kernel's indices cannot hold
                                    (ok, [0, 0], [30, 30], 10),          # one start per clip
                                    (ok, [0], [30], 0),
                                    ([], [], [], 10)):
        with pytest.raises(ValueError):
            gd.wave_descriptors(meta, starts, limits, n)
    # a CREMA-D clip shorter than a second: three copies do not fill the 3 s window
    with pytest.raises(ValueError, match="shorter spectrogram"):
        gd.wave_descriptors([(22049, 1, 0)], [0], [gd.wave_limit(22049, ("times", 3))], 66150)


@pytest.mark.parametrize("length", [1, 7, 159, 160, 161, 400])
def test_tiling_is_the_periodic_extension(length):
    """np.tile(...)[start:start + n] of either rule equals mono[(start + p) mod len] -- for every start the window fits at, at a
    toy rate of 16 Hz (ten seconds = 160 samples), on int16 stereo data so that the decode and the mix-down are in it."""
    rng = np.random.default_rng(length)
    raw = rng.integers(-32768, 32768, (length, 2)).astype(np.int16)
    for tiling, n in ((("double", 160), 80), (("times", 3), min(3 * length, 50))):
        limit = gd.wave_limit(length, tiling)
        for start in sorted({0, 1, length - 1, length, (limit - n) // 2, limit - n}):
            if 0 <= start <= limit - n:
                np.testing.assert_array_equal(wr.stage(raw, start, n, tiling), wr.stage_modulo(raw, start, n))


def test_decode_and_mixdown_restatement():
    """x / 32768 is exact in float32 and (l + r) / 2 is np.mean's float32 result for two channels."""
    raw = np.array([[-32768, 32767], [32767, 32767], [-32768, -32768], [1, -2], [12345, -54]], np.int16)
    got = wr.mono(wr.decode(raw))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.astype(np.float64), (raw[:, 0].astype(np.float64) + raw[:, 1]) / 65536.0)
    f = np.random.default_rng(0).standard_normal((1000, 2)).astype(np.float32)
    np.testing.assert_array_equal(wr.mono(f), (f[:, 0] + f[:, 1]) / np.float32(2))
    # and the staged window of such a clip is that mean, at the dataset's tiled length, clipped
    st = gd.AUDIO_STAGES["AVE"]
    limit = gd.wave_limit(len(f), st["tiling"])
    w = wr.stage(f, limit - 1200, 1200, st["tiling"])
    np.testing.assert_array_equal(w, np.clip(((f[:, 0] + f[:, 1]) / np.float32(2))[(limit - 1200 + np.arange(1200)) % 1000], -1, 1))
    assert w.min() == -1.0 and w.max() == 1.0


def test_random_wave_starts():
    g = torch.Generator().manual_seed(3)
    s = gd.random_wave_starts(20000, 5, generator=g)
    assert s.dtype == torch.int64 and sorted(set(s.tolist())) == [0, 1, 2, 3, 4, 5]  # `high` is included, like random.randint
    assert torch.equal(s, gd.random_wave_starts(20000, 5, generator=torch.Generator().manual_seed(3)))
    assert gd.random_wave_starts(4, 0).tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        gd.random_wave_starts(4, -1)


def test_abi_refuses_bad_arguments_without_a_gpu():
    """Every refusal of the header, with pointers that are never dereferenced: the host checks come before the launch."""
    assert L.SIGNATURES["gdl_wave_logspec"] == ("i", "pzp" + "iiiiiii" + "ppp")
    lib = L.load()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.addressof(buf)
    good = dict(src=p, src_bytes=64, desc=p, B=1, n=100, n_fft=64, hop=16, pad=0, oh=0, ow=0, wave=None, out=p)

    def rc(**kw):
        a = {**good, **kw}
        return lib.gdl_wave_logspec(a["src"], a["src_bytes"], a["desc"], a["B"], a["n"], a["n_fft"], a["hop"], a["pad"], a["oh"], a["ow"],
                                    a["wave"], a["out"], None)

    for kw in (dict(src=None), dict(desc=None), dict(out=None), dict(B=0), dict(B=-1), dict(n=0), dict(hop=0), dict(src_bytes=0),
               dict(n_fft=48), dict(n_fft=8), dict(n_fft=4096), dict(pad=2),
               dict(pad=1, n=32),              # reflect padding needs more than n_fft / 2 samples
               dict(oh=224), dict(ow=224),     # exactly one of the two
               dict(oh=-1, ow=-1), dict(oh=-224, ow=224),
               dict(src=p + 2), dict(src=p + 1),  # clips are read as dwords
               dict(desc=p + 4),
               dict(B=65536)):
        assert rc(**kw) != 0, kw
        assert b"wave_logspec" in lib.gdl_last_error(), kw


def test_no_cpu_path():
    host16 = torch.zeros(200000, dtype=torch.int16)
    for fn in (lambda: gd.stage_audio([host16], "KineticSound"),
               lambda: gd.stage_audio([host16.float()], "CREMAD"),
               lambda: gd.wave_log_spectrogram([host16], 1000, [0], [200000], 64, 16),
               lambda: gd.stage_audio((host16, torch.tensor([[0, 200000, 1, 1, 0, 200000]])), "KineticSound")):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(ValueError):
        gd.stage_audio([host16], "no such dataset")
    import gdl

    assert gdl.stage_audio is gd.stage_audio and gdl.wave_log_spectrogram is gd.wave_log_spectrogram
    assert gdl.wave_descriptors is gd.wave_descriptors and gdl.AUDIO_STAGES is gd.AUDIO_STAGES
    assert gdl.random_wave_starts is gd.random_wave_starts
