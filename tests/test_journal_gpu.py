"""GPU tests of the step journal (csrc/journal.hip): the kernel through the C ABI -- the ring, the cursor, the copied columns,
NaN for absent sources, the float64 epoch sums, run-to-run identical bits, nothing written outside the buffer -- and the two
runners with the switch on: each row against `read()` at that step, overflow, reset, every column family, and the step
bit-identical to the switch off.

Bound of the abs_out_a / abs_out_v columns against the float64 mean of the same float32 values (journal_ref.abs_mean_bound),
derived from the kernel's summation shape, not fitted: the block has 256 threads; a value passes through at most
ceil(n / 256) additions along its thread's strided chain, six butterfly levels in its wave and two for (w0 + w1) + (w2 + w3),
then one division by (float)n (exact for n < 2^24).  Every term is non-negative, so no partial sum exceeds the total and each
operation contributes at most one rounding of relative size 2^-24 (first order): (ceil(n / 256) + 8 + 1) 2^-24 in all.

Worst deviations measured on MI355X, as fractions of that bound: see docs/parity_log.md, "Step journal"."""
import argparse

import numpy as np
import pytest
import torch

import journal_ref as jr
from gdl import _lib as L
from gpu_util import DEV, dev
from oracle import fixtures as fx

pytestmark = pytest.mark.gpu

CAP, APPENDS, GUARD = 4, 6, 256
N_LOGITS = [1, 255, 256, 257, 384, 1236, 65537]  # block-size edges, one element, 64 x 6, 4 x 309, a long per-thread chain
WORST = {}
_SRC = {}


def _note(what, dev_, bound):
    WORST[what] = max(WORST.get(what, 0.0), dev_ / bound)
    print(f"journal deviation [{what}]: {dev_:.3e} of bound {bound:.3e} ({dev_ / bound:.3f}); worst ratio so far {WORST[what]:.3f}")


def _sources(n):
    """the six appends' sources for n_logits = n, made once (host float32 + device copies), never modified"""
    if n not in _SRC:
        r = np.random.default_rng([77, n])
        host = dict(losses=r.random((APPENDS, 3), dtype=np.float32) * 3, stats=r.random((APPENDS, 4), dtype=np.float32) * 40,
                    out_a=r.standard_normal((APPENDS, n), dtype=np.float32) * 2,
                    out_v=r.standard_normal((APPENDS, n), dtype=np.float32) * 5 + 1,
                    div=r.random((APPENDS, 2), dtype=np.float32) + 1, ogm=r.random((APPENDS, 5), dtype=np.float32))
        _SRC[n] = (host, {k: dev(v) for k, v in host.items()})
    return _SRC[n]


# which sources append i has: (one loss only, out_a, out_v, div_a, div_v, ogm)
_FULL = [(False, True, True, True, True, True)] * APPENDS
_SPARSE = [(False, True, True, True, True, False), (False, False, True, True, False, True), (False, True, False, True, True, True),
           (False, True, True, False, True, True), (False, False, False, True, True, False), (True, True, True, True, True, True)]


def _run(n, plan):
    """six appends into a zeroed capacity-4 buffer with guard bytes behind it; returns the buffer's bytes after each append"""
    host, d = _sources(n)
    nbytes = L.load().gdl_journal_bytes(CAP)
    assert nbytes == jr.HEADER_BYTES + CAP * 64
    buf = torch.zeros(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    buf[nbytes:] = 0xAB
    st = L.cur_stream()
    snaps = []
    for i, (one, oa, ov, da, dv, og) in enumerate(plan):
        no = not (oa or ov)
        L.call("gdl_journal_append", buf.data_ptr(), CAP, d["losses"][i].data_ptr(), 1 if one else 3, d["stats"][i].data_ptr(),
               d["out_a"][i].data_ptr() if oa else None, d["out_v"][i].data_ptr() if ov else None, 0 if no else n,
               d["div"][i].data_ptr() if da else None, d["div"][i].data_ptr() + 4 if dv else None,
               d["ogm"][i].data_ptr() if og else None, st)
        snaps.append(buf.cpu().numpy())
    return snaps


def _parts(h):
    nbytes = jr.HEADER_BYTES + CAP * 64
    return (int(h[:8].view(np.int64)[0]), h[8:32], h[jr.ACC_AT:jr.ACC_AT + 96].view(np.float64),
            h[jr.HEADER_BYTES:nbytes].view(np.float32).reshape(CAP, 16), h[nbytes:])


@pytest.mark.parametrize("plan", ["full", "sparse"])
@pytest.mark.parametrize("n", N_LOGITS)
def test_kernel_through_the_abi(n, plan):
    """capacity 4, six appends whose sources change every time: after append i the count is i + 1, row i % 4 holds that
    append's values (copies bit-equal, NaN for a NULL source, the two means within the derived bound of float64) and the other
    rows are untouched; the sums equal the sequential float64 sums of the rows bit for bit; the reserved words and the bytes
    behind the buffer are untouched; a second run from a zeroed buffer gives identical bits everywhere."""
    host, _ = _sources(n)
    pl = _FULL if plan == "full" else _SPARSE
    snaps = _run(n, pl)
    bound = jr.abs_mean_bound(n)
    rows_seen, prev = [], None
    for i, (h, (one, oa, ov, da, dv, og)) in enumerate(zip(snaps, pl)):
        count, reserved, acc, rows, guard = _parts(h)
        assert count == i + 1 and not reserved.any() and (guard == 0xAB).all() and acc[11] == 0.0
        want = jr.make_row(host["losses"][i][:1] if one else host["losses"][i], host["stats"][i],
                           host["out_a"][i] if oa else None, host["out_v"][i] if ov else None,
                           host["div"][i][0] if da else None, host["div"][i][1] if dv else None, host["ogm"][i] if og else None)
        got = rows[i % CAP]
        copied = [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15]
        assert jr.same_bits(got[copied], want[copied]), (i, got, want)
        for c, have, x in ((7, oa, host["out_a"][i]), (8, ov, host["out_v"][i])):
            if not have:
                assert np.isnan(got[c])
                continue
            ref = jr.abs_mean64(x)
            _note(f"kernel n={n}", abs(float(got[c]) - ref) / ref, bound)
            assert abs(float(got[c]) - ref) <= bound * ref, (i, c, got[c], ref)
        if prev is not None:  # the other three rows are as they were
            keep = [s for s in range(CAP) if s != i % CAP]
            assert rows[keep].tobytes() == prev[keep].tobytes()
        prev = rows.copy()
        rows_seen.append(got.copy())
        assert jr.same_bits(acc[:11], jr.acc_of(np.stack(rows_seen))), (i, acc, jr.acc_of(np.stack(rows_seen)))
    count, _, acc, rows, _ = _parts(snaps[-1])
    assert count == APPENDS
    for slot, step in jr.ring_slots(APPENDS, CAP):  # steps 2 .. 5 are retained, where the ring says
        assert rows[slot].tobytes() == rows_seen[step].tobytes()
    if plan == "sparse":  # a column that once had no source has a NaN sum; the others are numbers
        assert np.isnan(acc[7:11]).all() and np.isfinite(acc[:7]).all()
    else:
        assert np.isfinite(acc[:11]).all()
    again = _run(n, pl)
    for a, b in zip(snaps, again):
        assert a.tobytes() == b.tobytes()


def test_header_reset_and_large_capacity():
    """zeroing the first 128 bytes starts a new epoch (the rows need no clearing); the cursor is 64-bit"""
    host, d = _sources(384)
    cap = 3
    buf = torch.zeros(L.load().gdl_journal_bytes(cap), dtype=torch.uint8, device=DEV)

    def append(i):
        L.call("gdl_journal_append", buf.data_ptr(), cap, d["losses"][i].data_ptr(), 3, d["stats"][i].data_ptr(), None, None, 0,
               None, None, None, L.cur_stream())

    for i in range(5):
        append(i)
    buf[:jr.HEADER_BYTES].zero_()
    append(5)
    h = buf.cpu().numpy()
    assert int(h[:8].view(np.int64)[0]) == 1
    rows = h[jr.HEADER_BYTES:].view(np.float32).reshape(cap, 16)
    assert rows[0, :3].tobytes() == host["losses"][5].tobytes() and rows[1, :3].tobytes() == host["losses"][4].tobytes()
    acc = h[jr.ACC_AT:jr.ACC_AT + 88].view(np.float64)
    assert acc[:3].tobytes() == host["losses"][5].astype(np.float64).tobytes()
    # a count beyond 2^32: the slot is count % capacity in 64-bit arithmetic
    big = (1 << 33) + 2
    buf[:8] = torch.from_numpy(np.array([big], dtype=np.int64).view(np.uint8)).to(DEV)
    append(1)
    h = buf.cpu().numpy()
    assert int(h[:8].view(np.int64)[0]) == big + 1
    rows = h[jr.HEADER_BYTES:].view(np.float32).reshape(cap, 16)
    assert rows[big % cap, :3].tobytes() == host["losses"][1].tobytes()


# ------------------------------------------------------------------ the runners
_STATE = {}
_TINY = dict(dataset="CREMAD", n_classes=6, spec_hw=[65, 47], frames=2, image_hw=[64, 64], batch=4, seed=0, lr=2e-3, alpha=4.0)
_BATCH = {}


def _state(name):
    if name not in _STATE:
        P, Bf = fx.model_state(6, name)
        _STATE[name] = {k: torch.from_numpy(np.array(v)) for k, v in {**P, **Bf}.items()}
    return _STATE[name]


def _make_model(fusion, joint=False):
    from models.basic_model import AVClassifier, AVClassifier_DGL

    args = argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality="full", batch_size=4)
    model = (AVClassifier if joint else AVClassifier_DGL)(args)
    model.load_state_dict(_state("concat" if joint and fusion == "concat" else fusion + "_dgl"), strict=True)
    model = model.to(DEV)
    model.audio_net.gdl_dtype = "f32"
    model.visual_net.gdl_dtype = "f32"
    return model.train()


def _batch(st):
    if st not in _BATCH:
        c = _TINY
        spec, image, label = fx.make_batch(c["seed"] + st, c["batch"], c["spec_hw"], c["frames"], c["image_hw"], c["n_classes"])
        _BATCH[st] = (dev(spec), dev(image), torch.from_numpy(label).to(DEV))
    return _BATCH[st]


def _dgl(fusion, joint=False, **kw):
    from gdl.trainer import DGLTrainer

    kw.setdefault("alpha", _TINY["alpha"])
    return DGLTrainer(_make_model(fusion, joint), lr=_TINY["lr"], mode="joint" if joint else "dgl", **kw)


def _uni(modality, **kw):
    from gdl.unimodal import UnimodalTrainer
    from models.basic_model import AVClassifier_DGL

    model = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality=modality, batch_size=4))
    st = {k: v for k, v in _state("concat_dgl").items() if k.startswith(("fusion_module.", modality + "_net."))}
    st.update({k: torch.from_numpy(v) for k, v in fx.make_state({modality + "_classifier.weight": (6, 512),
                                                                  modality + "_classifier.bias": (6,)}).items()})
    model.load_state_dict(st, strict=True)
    model = model.to(DEV).train()
    getattr(model, modality + "_net").gdl_dtype = "f32"
    return UnimodalTrainer(model, lr=_TINY["lr"], **kw)


def _steps(tr, nsteps, before=None):
    """`nsteps` steps; after each, read() and the journal without a reset: (reads, that step's row as the journal holds it)"""
    reads, rows = [], []
    for st in range(nsteps):
        if before is not None:
            before(tr, st)
        tr.step(*_batch(st))
        reads.append(tr.read())
        j = tr.journal(reset=False)
        assert j["count"] == st + 1 and j["first_step"] + j["rows"].shape[0] == st + 1
        rows.append(j["rows"][-1].copy())
    return reads, np.stack(rows)


def _check_rows(what, reads, rows, logits):
    """every row against read() at its step: columns 0-6, 9-10 and 11-15 bit-equal to read()'s values as float32 (NaN where
    read() has no such key), 7-8 within the derived bound of the float64 mean |out_a| / |out_v| (NaN without unimodal logits)"""
    for r, row in zip(reads, rows):
        og = r.get("ogm")
        want = jr.make_row([r["loss_f"], r["loss_a"], r["loss_v"]],
                           [r["total_norm"], r["clip_coef"], r["audio_grad_sum"], r["visual_grad_sum"]],
                           div_a=r.get("a_diversity"), div_v=r.get("v_diversity"),
                           ogm=None if og is None else [og[k] for k in jr.COLUMNS[11:]])
        keep = [c for c in range(16) if c not in (7, 8)]
        assert jr.same_bits(row[keep], want[keep]), (what, row, want)
        for c, key in ((7, logits[0]), (8, logits[1])):
            if key is None:
                assert np.isnan(row[c])
                continue
            ref, bound = jr.abs_mean64(r[key]), jr.abs_mean_bound(r[key].size)
            _note(what, abs(float(row[c]) - ref) / ref, bound)
            assert abs(float(row[c]) - ref) <= bound * ref, (what, c, row[c], ref)


def _check_means(j, all_rows, fed):
    """means: the sequential float64 sums of ALL the steps' rows over the count, bit for bit, for exactly the columns fed"""
    want = jr.means_of(all_rows)
    assert set(j["means"]) == set(fed), (sorted(j["means"]), sorted(fed))
    for k in fed:
        assert jr.same_bits(np.float64(j["means"][k]), np.float64(want[k])), (k, j["means"][k], want[k])


_BASE = jr.COLUMNS[:7]
_MODES = {"dgl-concat": (dict(fusion="concat"), ("out_a", "out_v")), "dgl-sum": (dict(fusion="sum"), ("out_a", "out_v")),
          "joint-concat": (dict(fusion="concat", joint=True), (None, None))}


@pytest.mark.parametrize("which", list(_MODES))
def test_row_against_read(which):
    """journal=8, five steps, read() after each: the DGL step with the concat and the sum head, and the joint concat step,
    whose loss_a / loss_v columns are what read() reports and whose abs_out columns are NaN"""
    import gdl.journal as gj

    kw, logits = _MODES[which]
    tr = _dgl(journal=8, **kw)
    reads, rows = _steps(tr, 5)
    _check_rows(which, reads, rows, logits)
    j = tr.journal(reset=False)
    assert j["columns"] == gj.COLUMNS and j["rows"].dtype == np.float32 and j["rows"].shape == (5, 16)
    assert (j["first_step"], j["count"], j["dropped"]) == (0, 5, 0)
    assert j["rows"].tobytes() == rows.tobytes()
    assert np.isnan(j["rows"][:, 9:]).all()  # no diversity monitor, no modulation
    _check_means(j, rows, _BASE + (("abs_out_a", "abs_out_v") if logits[0] else ()))
    for k, col in (("loss_f", 0), ("audio_grad_sum", 5)):  # and against the read() values themselves
        assert j["means"][k] == jr.seq_sum([np.float32(r[k]) for r in reads]) / 5
    tr.close()


def test_overflow_and_reset():
    """journal=2, five steps: the rows are those of steps 3 and 4, three were dropped, the means still cover all five; reset=False
    keeps everything, reset=True leaves count 0 and NaN means, and the next epoch starts from there"""
    tr = _dgl("concat", journal=2)
    reads, rows = _steps(tr, 5)
    _check_rows("overflow", reads, rows, ("out_a", "out_v"))
    fed = _BASE + ("abs_out_a", "abs_out_v")
    for _ in range(2):  # reset=False changes nothing
        j = tr.journal(reset=False)
        assert (j["first_step"], j["count"], j["dropped"]) == (3, 5, 3)
        assert j["rows"].tobytes() == rows[3:].tobytes()
        _check_means(j, rows, fed)
    j = tr.journal()  # the same once more, then reset
    assert j["count"] == 5 and j["rows"].tobytes() == rows[3:].tobytes()
    j = tr.journal(reset=False)
    assert (j["count"], j["dropped"]) == (0, 0) and j["rows"].shape == (0, 16) and j["first_step"] == 5
    assert set(j["means"]) == set(fed) and all(np.isnan(v) for v in j["means"].values())
    tr.step(*_batch(5))
    r = tr.read()
    j = tr.journal()
    assert (j["first_step"], j["count"], j["dropped"]) == (5, 1, 0)
    _check_rows("after reset", [r], j["rows"], ("out_a", "out_v"))
    _check_means(j, j["rows"], fed)
    tr.close()


def _snapshot(tr, r):
    keys = ("loss_f", "loss_a", "loss_v", "total_norm", "clip_coef", "audio_grad_sum", "visual_grad_sum")
    opt = np.concatenate([v.cpu().numpy() for v in tr._opt_state().values()])
    return {"params": tr.params.cpu().numpy(), "grads": tr.grads.cpu().numpy(), "opt": opt, "out": r["out"],
            "out_a": r["out_a"], "out_v": r["out_v"], "scalars": np.array([r[k] for k in keys], dtype=np.float64),
            "grad_norm": np.array(list(r["grad_norm"].values())), "grad_absmean": np.array(list(r["grad_absmean"].values()))}


def test_on_against_off():
    """two trainers from the same state, three steps: parameters, optimizer state, gradients and read() are bit-identical with
    journal=4 and journal=0; off, nothing is allocated, read() has the same keys and journal() raises"""
    snaps, keys = {}, {}
    for cap in (0, 4):
        tr = _dgl("concat", journal=cap)
        for st in range(3):
            tr.step(*_batch(st))
        r = tr.read()
        snaps[cap], keys[cap] = _snapshot(tr, r), set(r)
        if cap == 0:
            assert tr._journal is None
            with pytest.raises(L.GdlError, match="off"):
                tr.journal()
        else:
            assert tr.journal()["count"] == 3
        tr.close()
    assert keys[0] == keys[4]
    for k in snaps[0]:
        assert snaps[0][k].tobytes() == snaps[4][k].tobytes(), k


def test_diversity_columns():
    """diversity=True: columns 9-10 are read()'s a_diversity / v_diversity bit for bit and have means; off they are NaN and
    absent from the means (test_row_against_read)"""
    tr = _dgl("concat", journal=4, diversity=True)
    reads, rows = _steps(tr, 3)
    assert all("a_diversity" in r and "v_diversity" in r for r in reads) and np.isfinite(rows[:, 9:11]).all()
    _check_rows("diversity", reads, rows, ("out_a", "out_v"))
    j = tr.journal()
    _check_means(j, rows, _BASE + ("abs_out_a", "abs_out_v", "a_diversity", "v_diversity"))
    ep = tr.epoch_diversity()  # the monitor's own float32 epoch mean is close to the journal's float64 one
    assert abs(ep["a_diversity"] - j["means"]["a_diversity"]) <= 1e-6 * j["means"]["a_diversity"]
    tr.close()


def test_ogm_columns():
    """mode="joint", modulation="OGM", alpha=0.8: columns 11-15 are read()["ogm"] bit for bit on a modulated step, NaN once
    tr.epoch lies beyond modulation_ends; the abs_out columns are NaN (the joint step has no unimodal logits)"""
    tr = _dgl("concat", joint=True, journal=4, modulation="OGM", alpha=0.8, modulation_ends=50)

    def before(t, st):
        if st == 2:
            t.epoch = 51

    reads, rows = _steps(tr, 3, before)
    assert "ogm" in reads[0] and "ogm" in reads[1] and "ogm" not in reads[2]
    assert np.isfinite(rows[:2, 11:]).all() and np.isnan(rows[2, 11:]).all()
    _check_rows("ogm", reads, rows, (None, None))
    j = tr.journal()
    _check_means(j, rows, _BASE)
    tr.close()


def test_unimodal():
    """UnimodalTrainer (audio), journal=4, three steps: the one loss in columns 0-2, audio_grad_sum as read() has it, a
    visual_grad_sum of 0.0, mean |out| in both abs_out columns"""
    tr = _uni("audio", journal=4)
    reads, rows = [], []
    for st in range(3):
        tr.step(*_batch(st))
        reads.append(tr.read())
    j = tr.journal()
    rows = j["rows"]
    assert (j["first_step"], j["count"], j["dropped"]) == (0, 3, 0) and rows.shape == (3, 16)
    for r, row in zip(reads, rows):
        loss = np.float32(r["loss_f"])
        assert row[0].tobytes() == loss.tobytes() and row[1].tobytes() == loss.tobytes() and row[2].tobytes() == loss.tobytes()
        assert row[3].tobytes() == np.float32(r["total_norm"]).tobytes() and row[4].tobytes() == np.float32(r["clip_coef"]).tobytes()
        assert row[5].tobytes() == np.float32(r["audio_grad_sum"]).tobytes() and row[5] > 0
        assert row[6].tobytes() == np.float32(0.0).tobytes()
        assert row[7].tobytes() == row[8].tobytes()
        ref, bound = jr.abs_mean64(r["out"]), jr.abs_mean_bound(r["out"].size)
        _note("unimodal", abs(float(row[7]) - ref) / ref, bound)
        assert abs(float(row[7]) - ref) <= bound * ref
        assert np.isnan(row[9:]).all()
    _check_means(j, rows, _BASE + ("abs_out_a", "abs_out_v"))
    tr.close()
    off = _uni("audio")
    with pytest.raises(L.GdlError, match="off"):
        off.journal()
    off.close()
