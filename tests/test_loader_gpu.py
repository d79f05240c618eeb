"""The device-resident epoch loader on the GPU: gdl_loader_plan's four tables against the NumPy restatement tests/loader_ref.py,
exactly (test_loader_cpu.py shows that none of the compared tries is decided by less than 8 ulp, and every comparison here asserts
it again for its own plan); gdl.DeviceLoader's batches bit for bit against gdl.data's host API fed the restatement's draws; the
epoch's coverage, the rank partition, determinism across depth / stream / resume; two trainer steps; the refusals."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loader_ref as lr  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gdl import data as gd  # noqa: E402
from gpu_util import DEV  # noqa: E402

SEED, EPOCH = lr.TOY_SEEDS[0], lr.TOY_EPOCHS[1]
AUDIO, SIZE, START_HIGH = lr.TOY_AUDIO, lr.TOY_SIZE, lr.TOY_AUDIO["start_high"]
TABLES = ("index", "label", "wave_desc", "crop_desc")
CANARY, GUARD = -0x5A5A5A5A5A5A5A5B, 16


def _draw(scale=lr.DEFAULT_SCALE, ratio=lr.DEFAULT_RATIO, p_flip=lr.DEFAULT_P_FLIP):
    return (ctypes.c_double * 7)(*lr.draw_params(scale, ratio, p_flip))


def _plan_abi(tabs, N, T, seed, epoch, first, count, shuffle, augment, rows=None, ptrs=None, draw=None, n_samples=1000,
              start_high=START_HIGH, size=(SIZE, SIZE)):
    """gdl_loader_plan into tables of `rows` positions (default: count) with a guard of canaries behind each.  -> (rc, tables)"""
    rows = max(count, 1) if rows is None else rows
    out = {k: torch.full((rows * w + GUARD,), CANARY, dtype=torch.int64, device=DEV) for k, w in zip(TABLES, (1, 1, 6, 8 * T))}
    draw = _draw() if draw is None else draw
    p = dict(clips=L.ptr(tabs[0]), frames=L.ptr(tabs[1]), labels=L.ptr(tabs[2]), draw=ctypes.cast(draw, ctypes.c_void_p),
             **{k: L.ptr(v) for k, v in out.items()})
    p.update(ptrs or {})
    rc = L.load().gdl_loader_plan(p["clips"], p["frames"], p["labels"], N, T, seed, epoch, first, count, shuffle, augment, n_samples,
                                  start_high, size[0], size[1], p["draw"], p["index"], p["label"], p["wave_desc"], p["crop_desc"],
                                  L.cur_stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _dev_tables(N, T):
    _, _, labels, clips, frames = lr.toy_layout(N, T)
    return (clips, frames, labels), tuple(torch.from_numpy(a).to(DEV) for a in (clips, frames, labels))


@pytest.mark.parametrize("N,T", lr.TOY_PLANNER_CASES)
def test_planner_tables_exact(N, T):
    host, tabs = _dev_tables(N, T)
    widths = dict(index=1, label=1, wave_desc=6, crop_desc=8 * T)
    for seed in lr.TOY_SEEDS[:1] if N == 1000 else lr.TOY_SEEDS:
        for epoch in lr.TOY_EPOCHS:
            for shuffle in (0, 1):
                for augment in (0, 1):
                    for first, count in lr.toy_ranges(N):
                        want = lr.plan(*host, T, seed, epoch, first, count, shuffle, augment, START_HIGH)
                        assert want["undecided"] == 0  # the condition of an exact comparison
                        rc, got = _plan_abi(tabs, N, T, seed, epoch, first, count, shuffle, augment)
                        assert rc == 0, L.last_error()
                        for k in TABLES:
                            n = count * widths[k]
                            np.testing.assert_array_equal(got[k][:n], want[k].reshape(-1), err_msg=str((k, seed, epoch, shuffle, augment, first)))
                            assert (got[k][n:] == CANARY).all(), k


def test_planner_range_in_two_calls():
    """Positions [0, 67) planned at once, and as [0, 29) + [29, 67): the same rows (a row depends on its position alone)."""
    N, T = 67, 3
    _, tabs = _dev_tables(N, T)
    _, full = _plan_abi(tabs, N, T, SEED, EPOCH, 0, N, 1, 1)
    _, a = _plan_abi(tabs, N, T, SEED, EPOCH, 0, 29, 1, 1)
    _, b = _plan_abi(tabs, N, T, SEED, EPOCH, 29, N - 29, 1, 1)
    for k, w in zip(TABLES, (1, 1, 6, 8 * T)):
        np.testing.assert_array_equal(np.concatenate([a[k][:29 * w], b[k][:(N - 29) * w]]), full[k][:N * w])
    assert sorted(full["index"][:N].tolist()) == list(range(N))


def test_planner_argument_errors_launch_nothing():
    N, T = 67, 3
    _, tabs = _dev_tables(N, T)
    ok = dict(N=N, T=T, first=0, count=N, shuffle=1, augment=1)
    bad = [dict(first=1), dict(first=-1, count=5), dict(count=0), dict(count=-3), dict(first=N, count=1), dict(N=0), dict(N=1 << 31),
           dict(T=0), dict(T=65), dict(shuffle=2), dict(augment=-1), dict(ptrs=dict(index=None)), dict(ptrs=dict(clips=None)),
           dict(ptrs=dict(label=L.ptr(tabs[2]) + 4)), dict(n_samples=0), dict(start_high=-1), dict(start_high=1 << 31),
           dict(size=(0, 32)), dict(draw=_draw(scale=(0.5, 0.1))), dict(draw=_draw(p_flip=1.5)), dict(ptrs=dict(draw=None))]
    for change in bad:
        kw = {**ok, **change}
        extra = {k: kw.pop(k) for k in ("ptrs", "draw", "n_samples", "start_high", "size") if k in kw}
        rc, got = _plan_abi(tabs, kw["N"], kw["T"], SEED, EPOCH, kw["first"], kw["count"], kw["shuffle"], kw["augment"], rows=N, **extra)
        assert rc == 1 and L.last_error(), change  # GDL_ERR_ARG
        for k in TABLES:
            assert (got[k] == CANARY).all(), (change, k)


# ------------------------------------------------------------------------------------------------ the loader
def _make_dataset(N, T):
    import gdl

    meta, sizes, labels, clips_tab, frames_tab = lr.toy_layout(N, T)
    g = torch.Generator().manual_seed(100 * N + T)
    clips = []
    for n, ch, fmt in meta:
        if fmt == gd.GDL_WAVE_S16:
            clips.append(torch.randint(-32768, 32768, (n, ch), generator=g, dtype=torch.int32).to(torch.int16))
        else:
            clips.append(torch.randn(n, generator=g) * 0.7)
    frames = [[torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.int32).to(torch.uint8) for h, w in per] for per in sizes]
    ds = gdl.DeviceDataset(clips, frames, torch.from_numpy(labels), AUDIO, T, size=SIZE, device=DEV)
    # the tables are laid out as the restatement's toy says: every clip and frame on a dword, the limit by the tiling rule
    assert np.array_equal(ds.clips.cpu().numpy(), clips_tab) and np.array_equal(ds.frames.cpu().numpy(), frames_tab)
    assert np.array_equal(ds.labels.cpu().numpy(), labels) and len(ds) == N
    assert ds.nbytes == ds.wave.numel() + ds.pixels.numel() + 8 * (5 * N + 3 * N * T + N)
    return dict(ds=ds, clips=[c.to(DEV) for c in clips], frames=[[f.to(DEV) for f in per] for per in frames], labels=labels,
                host=(clips_tab, frames_tab, labels), N=N, T=T)


@pytest.fixture(scope="module")
def toy13():
    return _make_dataset(13, 3)


@pytest.fixture(scope="module")
def toy67():
    return _make_dataset(67, 1)


def _loader(toy, B, train=True, seed=SEED, epoch=EPOCH, **kw):
    import gdl

    ld = gdl.DeviceLoader(toy["ds"], B, train, seed=seed, **kw)
    ld.set_epoch(epoch)
    return ld


def _take(ld):
    """Every batch of the epoch, cloned as it is taken."""
    return [tuple(t.clone() for t in batch) for batch in ld]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for ba, bb in zip(a, b) for x, y in zip(ba, bb))


@pytest.mark.parametrize("train", [True, False])
def test_loader_batches_equal_the_host_api(toy13, train):
    """A batch = resized_crop_frames + wave_log_spectrogram of the host API fed the restatement's indices, boxes, flips and starts;
    in eval mode = augment_frames(train=False) of the samples in file order (and the drawn window)."""
    N, T, B = toy13["N"], toy13["T"], 4
    ld = _loader(toy13, B, train)
    assert len(ld) == 3
    want = lr.plan(*toy13["host"], T, SEED, EPOCH, 0, 12, int(train), int(train), START_HIGH)
    assert want["undecided"] == 0
    got = ld.plan()
    for k in TABLES:
        np.testing.assert_array_equal(got[k].numpy().reshape(-1), want[k].reshape(-1), err_msg=k)
    batches = _take(ld)
    assert len(batches) == 3
    for k, (spec, image, label) in enumerate(batches):
        idx = want["index"][k * B:(k + 1) * B].tolist()
        if not train:
            assert idx == list(range(k * B, (k + 1) * B))
        frames = [toy13["frames"][i][t] for i in idx for t in range(T)]
        rows = want["crop_desc"][k * B * T:(k + 1) * B * T]
        if train:
            want_image = gd.resized_crop_frames(frames, rows[:, 3:7], rows[:, 7], size=SIZE, T=T)
        else:
            want_image = gd.augment_frames(frames, T, False, size=SIZE)
        wrows = want["wave_desc"][k * B:(k + 1) * B]
        want_spec = gd.wave_log_spectrogram([toy13["clips"][i] for i in idx], AUDIO["n_samples"], wrows[:, 4], wrows[:, 5],
                                            AUDIO["n_fft"], AUDIO["hop_length"])
        assert image.dtype == torch.float32 and tuple(image.shape) == (B, 3, T, SIZE, SIZE) and torch.isfinite(image).all()
        assert spec.dtype == torch.float32 and tuple(spec.shape) == (B, 33, 63)
        assert torch.equal(image, want_image) and torch.equal(spec, want_spec)
        assert label.dtype == torch.int64 and label.tolist() == toy13["labels"][idx].tolist()
    if train:
        assert want["crop_desc"][:, 7].min() == 0 and want["crop_desc"][:, 7].max() == 1  # both flips, and the fallback sample
        assert 6 in want["index"]


def test_epoch_coverage_ranks_and_batch_size(toy67):
    N = toy67["N"]
    p4 = _loader(toy67, 4).plan()
    idx4 = p4["index"].tolist()
    assert len(_loader(toy67, 4)) == 16 and len(idx4) == 64 and len(set(idx4)) == 64 and set(idx4) <= set(range(N))
    assert idx4 != sorted(idx4) and idx4 != _loader(toy67, 4, epoch=EPOCH + 1).plan()["index"].tolist()
    # batch size 8: fewer, larger batches over the same order, and every sample keeps its window, box and flip
    p8 = _loader(toy67, 8).plan()
    assert p8["index"].tolist() == idx4
    for k in TABLES:
        assert torch.equal(p4[k], p8[k])
    b4, b8 = _take(_loader(toy67, 4)), _take(_loader(toy67, 8))
    for j in range(3):
        assert torch.equal(torch.cat([b[j] for b in b4]), torch.cat([b[j] for b in b8]))
    # two ranks partition the positions: rank r's batch k is positions (2 k + r) * 4 ..
    r0, r1 = _take(_loader(toy67, 4, rank=0, world_size=2)), _take(_loader(toy67, 4, rank=1, world_size=2))
    assert len(r0) == len(r1) == 8
    for k in range(8):
        assert _same([r0[k]], [b4[2 * k]]) and _same([r1[k]], [b4[2 * k + 1]])


def test_determinism_depth_stream_resume(toy67):
    base = _take(_loader(toy67, 8))
    assert len(base) == 8 and not torch.equal(base[0][1], base[1][1])
    assert _same(base, _take(_loader(toy67, 8)))
    assert not _same(base, _take(_loader(toy67, 8, seed=SEED + 1)))
    assert _same(base, _take(_loader(toy67, 8, depth=1))) and _same(base, _take(_loader(toy67, 8, depth=3)))
    side = torch.cuda.Stream(device=DEV)
    assert _same(base, _take(_loader(toy67, 8, stream=side))) and _same(base, _take(_loader(toy67, 8, stream=side, depth=3)))
    # the same loader again: the epoch rewinds; another epoch differs
    ld = _loader(toy67, 8, stream=side)
    assert _same(base, _take(ld)) and _same(base, _take(ld))
    ld.set_epoch(EPOCH + 1)
    assert not _same(base, _take(ld))
    # resume after batch 2
    first = _loader(toy67, 8)
    it = iter(first)
    head = [tuple(t.clone() for t in next(it)) for _ in range(2)]
    state = first.state_dict()
    assert state == dict(seed=SEED, epoch=EPOCH, next_batch=2)
    for kw in (dict(), dict(stream=side)):
        resumed = _loader(toy67, 8, seed=99, epoch=0, **kw)
        resumed.load_state_dict(state)
        assert _same(base, head + _take(resumed))


def test_two_trainer_steps_fed_by_the_loader():
    """test_ablation_gpu.py's tiny configuration (spec 65 x 47, two 64 x 64 frames, B = 4): a trainer stepped on the loader's
    views gives the logits and losses of the same trainer stepped on clones of those batches."""
    import gdl
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier_DGL
    from oracle import fixtures as fx

    N, T, B = 8, 2, 4
    g = torch.Generator().manual_seed(3)
    audio = dict(n_samples=4600, tiling=("times", 1), start_high=START_HIGH, n_fft=128, hop_length=100, resize=None)
    clips = [torch.randn(5000 + 13 * i, generator=g) * 0.5 for i in range(N)]
    frames = torch.randint(0, 256, (N, T, 64, 64, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    labels = torch.randint(0, 6, (N,), generator=g)
    ds = gdl.DeviceDataset(clips, frames, labels, audio, T, size=64, device=DEV)
    P, Bf = fx.model_state(6, "concat_dgl")
    state = {k: torch.from_numpy(np.array(v)) for k, v in {**P, **Bf}.items()}

    def run(clone):
        model = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=B))
        model.load_state_dict(state, strict=True)
        model = model.to(DEV)
        model.audio_net.gdl_dtype = model.visual_net.gdl_dtype = "f32"
        tr = DGLTrainer(model.train(), lr=2e-3, alpha=4.0)
        ld = gdl.DeviceLoader(ds, B, True, seed=SEED)
        ld.set_epoch(lr.TOY_EPOCHS[0])
        reads = []
        for spec, image, label in ld:
            assert tuple(spec.shape) == (B, 65, 47) and tuple(image.shape) == (B, 3, T, 64, 64)
            if clone:
                spec, image, label = spec.clone(), image.clone(), label.clone()
            tr.step(spec, image, label)
            reads.append(tr.read())
        return reads

    a, b = run(False), run(True)
    assert len(a) == len(b) == 2
    for ra, rb in zip(a, b):
        for k in ("out", "out_a", "out_v"):
            assert np.isfinite(ra[k]).all()
            np.testing.assert_array_equal(ra[k], rb[k])
        for k in ("loss_f", "loss_a", "loss_v"):
            assert np.isfinite(ra[k]) and ra[k] == rb[k]
    assert not np.array_equal(a[0]["out"], a[1]["out"])


def test_refusals(toy13):
    import gdl

    ds, T = toy13["ds"], toy13["T"]
    clips = [c.cpu() for c in toy13["clips"]]
    frames = [[f.cpu() for f in per] for per in toy13["frames"]]
    labels = torch.from_numpy(toy13["labels"])
    with pytest.raises(ValueError, match="GPU"):
        gdl.DeviceDataset(clips, frames, labels, AUDIO, T, size=SIZE, device="cpu")
    with pytest.raises(ValueError, match="DeviceDataset"):
        gdl.DeviceLoader(list(zip(clips, frames, labels.tolist())), 4, True)
    with pytest.raises(ValueError, match="sample 0 has 3 frames"):
        gdl.DeviceDataset(clips, frames, labels, AUDIO, 2, size=SIZE, device=DEV)
    with pytest.raises(ValueError, match="integers"):
        gdl.DeviceDataset(clips, frames, labels.float(), AUDIO, T, size=SIZE, device=DEV)
    with pytest.raises(ValueError, match="no audio stage"):
        gdl.DeviceDataset(clips, frames, labels, "no such dataset", T, size=SIZE, device=DEV)
    short = [c.clone() for c in clips]
    short[5] = short[5][:100]  # four copies of 100 samples hold no window of 37 + 1000; every other clip has 300 samples or more
    with pytest.raises(ValueError, match="clip 5"):
        gdl.DeviceDataset(short, frames, labels, dict(AUDIO, tiling=("times", 4)), T, size=SIZE, device=DEV)
    big = [[torch.zeros(2160, 3840, 3, dtype=torch.uint8)] * T if i == 2 else per for i, per in enumerate(frames)]
    with pytest.raises(ValueError, match="2160 x 3840 frames .first in sample 2"):
        gdl.DeviceDataset(clips, big, labels, AUDIO, T, size=224, device=DEV)
    for kw, what in ((dict(batch_size=14), "no full batch"), (dict(batch_size=7, world_size=2), "no full batch"),
                     (dict(batch_size=4, depth=0), "depth"), (dict(batch_size=4, rank=2, world_size=2), "rank"),
                     (dict(batch_size=4, depth=1, stream=torch.cuda.Stream(device=DEV)), "depth must be at least 2"),
                     (dict(batch_size=4, pad_mode="edge"), "pad_mode"), (dict(batch_size=4, scale=(1.0, 0.5)), "scale")):
        with pytest.raises(ValueError, match=what):
            gdl.DeviceLoader(ds, train=True, **kw)
    with pytest.raises(ValueError, match="device"):
        gdl.DeviceDataset.from_packed(ds.wave.cpu(), ds.clips, ds.pixels, ds.frames, ds.labels, AUDIO, T, size=SIZE)
    again = gdl.DeviceDataset.from_packed(ds.wave, ds.clips, ds.pixels, ds.frames, ds.labels, AUDIO, T, size=SIZE)
    assert again.nbytes == ds.nbytes and _same(_take(gdl.DeviceLoader(again, 4, True, seed=SEED)), _take(gdl.DeviceLoader(ds, 4, True, seed=SEED)))
    ld = gdl.DeviceLoader(ds, 4, True)
    with pytest.raises(L.GdlError, match="before iter"):
        next(ld)
    with pytest.raises(ValueError, match="next_batch"):
        ld.load_state_dict(dict(seed=0, epoch=0, next_batch=4))
