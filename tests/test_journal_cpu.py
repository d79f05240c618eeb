"""CPU-only checks of the step journal: the symbol and its binding, the column count, the buffer size, every refusal of the C
ABI (all decided on the host, before any launch), the NumPy restatement tests/journal_ref.py against direct NumPy, and the
trainers' `journal` argument."""
import argparse
import ctypes
import inspect
import re
import os

import numpy as np
import pytest

import journal_ref as jr
from gdl import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_signature():
    lib = L.load()
    for name in ("gdl_journal_bytes", "gdl_journal_append"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert L.SIGNATURES["gdl_journal_bytes"] == ("z", "l")
    fn = lib.gdl_journal_append
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 12
    # journal, capacity | losses, n_losses | stats | out_a, out_v, n_logits | div_a, div_v | ogm | stream
    want = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_int64] + [ctypes.c_void_p] * 4
    assert list(fn.argtypes) == want


def test_column_count_agrees_everywhere():
    import gdl
    import gdl.journal as gj

    with open(os.path.join(ROOT, "include", "gdl_hip.h")) as f:
        cols = int(re.search(r"^#define GDL_JOURNAL_COLS (\d+)$", f.read(), re.M).group(1))
    assert cols == len(gj.COLUMNS) == L.GDL_JOURNAL_COLS == 16
    assert gj.COLUMNS == jr.COLUMNS and gdl.journal is gj
    assert gj.COLUMNS[5:7] == ("audio_grad_sum", "visual_grad_sum")  # the script's CSV row
    assert (gj.N_ACC, gj.HEADER_BYTES) == (jr.N_ACC, jr.HEADER_BYTES)


def test_bytes():
    nb = L.load().gdl_journal_bytes
    assert nb(0) == 0 and nb(-3) == 0
    assert nb(1) == jr.HEADER_BYTES + 64
    for c in (1, 2, 7, 100, 1 << 20):
        assert nb(c + 1) - nb(c) == 64  # one row of 16 floats
    assert nb(1 << 34) == jr.HEADER_BYTES + 64 * (1 << 34)  # no 32-bit arithmetic


def test_refusals_need_no_gpu():
    lib = L.load()
    one = ctypes.c_void_p(256)  # never dereferenced: every case below is refused on the host

    def refused(match, journal=one, capacity=4, losses=one, n_losses=3, stats=one, out_a=one, out_v=one, n_logits=24, ogm=one):
        rc = lib.gdl_journal_append(journal, capacity, losses, n_losses, stats, out_a, out_v, n_logits, one, one, ogm, None)
        assert rc == 1 and match in lib.gdl_last_error(), (rc, lib.gdl_last_error())  # GDL_ERR_ARG

    refused(b"null journal", journal=None)
    refused(b"capacity", capacity=0)
    refused(b"capacity", capacity=-1)
    for n in (0, 2, 4, -1):
        refused(b"n_losses", n_losses=n)
    refused(b"null losses or stats", losses=None)
    refused(b"null losses or stats", stats=None)
    refused(b"n_logits", n_logits=-1)
    refused(b"n_logits = 0", n_logits=0)
    refused(b"n_logits = 0", n_logits=0, out_v=None)
    refused(b"n_logits = 0", n_logits=0, out_a=None)
    refused(b"aligned", journal=ctypes.c_void_p(264))


def test_ref_against_direct_numpy():
    r = np.random.default_rng(11)
    for n in (1, 24, 255, 257, 1236, 65537):
        x = (r.standard_normal(n) * 3).astype(np.float32)
        assert jr.abs_mean64(x) == float(np.mean(np.abs(x.astype(np.float64))))
    assert jr.abs_mean_bound(1) == 10 * 2.0 ** -24 and jr.abs_mean_bound(256) == 10 * 2.0 ** -24
    assert jr.abs_mean_bound(257) == 11 * 2.0 ** -24 and jr.abs_mean_bound(65537) == (257 + 9) * 2.0 ** -24
    losses, stats, ogm = r.random(3).astype(np.float32), r.random(4).astype(np.float32), r.random(5).astype(np.float32)
    oa, ov = r.standard_normal(24).astype(np.float32), r.standard_normal(24).astype(np.float32)
    row = jr.make_row(losses, stats, oa, ov, 1.5, 2.5, ogm)
    assert row.dtype == np.float32 and row.shape == (16,)
    want = np.concatenate([losses, stats, [np.abs(oa.astype(np.float64)).mean(), np.abs(ov.astype(np.float64)).mean(), 1.5, 2.5],
                           ogm]).astype(np.float32)
    assert row.tobytes() == want.tobytes()
    row = jr.make_row(losses[:1], stats)  # one loss in all three columns; every absent source is NaN
    assert (row[:3] == losses[0]).all() and row[3:7].tobytes() == stats.tobytes() and np.isnan(row[7:]).all()
    row = jr.make_row(losses, stats, out_v=ov, div_a=0.25)
    assert np.isnan(row[[7, 10]]).all() and np.isnan(row[11:]).all() and row[9] == 0.25 and np.isfinite(row[8])
    # the epoch sums: sequential float64, which is what math.fsum is NOT and what a float64 cumsum is
    rows = np.stack([jr.make_row(r.random(3), r.random(4), r.standard_normal(7), r.standard_normal(7), r.random(), r.random())
                     for _ in range(9)])
    acc = jr.acc_of(rows)
    assert acc.tobytes() == np.cumsum(rows[:, :11].astype(np.float64), axis=0)[-1].tobytes()
    m = jr.means_of(rows)
    assert list(m) == list(jr.COLUMNS[:11]) and m["loss_v"] == acc[2] / 9
    assert all(np.isnan(v) for v in jr.means_of(np.zeros((0, 16), np.float32)).values())
    rows[4, 9] = np.nan  # a NaN propagates into its own sum alone
    acc = jr.acc_of(rows)
    assert np.isnan(acc[9]) and np.isfinite(np.delete(acc, 9)).all()
    assert jr.ring_slots(6, 4) == [(2, 2), (3, 3), (0, 4), (1, 5)] and jr.ring_slots(3, 4) == [(0, 0), (1, 1), (2, 2)]
    assert jr.ring_slots(0, 4) == []
    a = np.array([1.0, np.nan, -0.0], np.float32)
    assert jr.same_bits(a, a.copy()) and not jr.same_bits(a, np.array([1.0, np.nan, 0.0], np.float32))
    assert not jr.same_bits(a, np.array([1.0, 2.0, -0.0], np.float32))


def test_python_surface_without_a_device():
    """both runners take `journal` (0 = off by default), refuse a capacity that is not a count before they touch the model, and
    still refuse a CPU model"""
    from gdl.trainer import DGLTrainer
    from gdl.unimodal import UnimodalTrainer
    from models.basic_model import AVClassifier_DGL

    for cls in (DGLTrainer, UnimodalTrainer):
        assert inspect.signature(cls.__init__).parameters["journal"].default == 0
        assert callable(cls.journal)
        for bad in (-1, 2.5, True, "8"):
            with pytest.raises(ValueError, match="journal"):
                cls(None, lr=1e-3, journal=bad)
    m = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=4))
    with pytest.raises(L.GdlError, match="cuda"):
        DGLTrainer(m, lr=1e-3, journal=8)
    ma = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="audio", batch_size=4))
    with pytest.raises(L.GdlError, match="cuda"):
        UnimodalTrainer(ma, lr=1e-3, journal=8)
