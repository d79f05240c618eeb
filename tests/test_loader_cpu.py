"""The arithmetic of gdl_loader_plan, on its NumPy restatement tests/loader_ref.py (no GPU): the keyed shuffle is a bijection and
spreads evenly, the crop boxes are torchvision's published RandomResizedCrop.get_params (inside the frame, inside the ratio
range, the fallback where no try fits), the window starts cover their range, the counters stay in the loader's own Philox
range -- and, as a condition of the exact GPU comparison in test_loader_gpu.py, none of the tries that file's seeds and frame
sizes produce is decided by less than 8 ulp."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loader_ref as lr  # noqa: E402

DRAW = lr.draw_params()


@pytest.mark.parametrize("N", [1, 2, 3, 5, 64, 67, 1000, 6698])
def test_permutation_is_a_bijection(N):
    pos = np.arange(N)
    orders = {}
    for seed, epoch in ((0, 0), (0, 1), (7, 0)):
        passes = []
        idx = lr.permute(pos, N, seed, epoch, passes)
        assert idx.dtype == np.int64 and np.array_equal(np.sort(idx), pos), (N, seed, epoch)
        assert passes[0] < 64  # (cycle walking: under 4 passes on average; the prototype's longest walk was 18)
        orders[seed, epoch] = idx
    assert np.array_equal(lr.permute(pos, N, 0, 0), orders[0, 0])  # a function of (seed, epoch, position)
    if N >= 64:  # two epochs and two seeds give different orders
        assert not np.array_equal(orders[0, 0], orders[0, 1]) and not np.array_equal(orders[0, 0], orders[7, 0])
    assert lr.kbits(N) == max(1, -(-(N - 1).bit_length() // 2)) and 4 ** lr.kbits(N) >= N


def test_permutation_spreads_evenly():
    """position -> index over 4 000 epochs at N = 16: Pearson's chi-squared on the 16 x 16 table of counts, 225 degrees of freedom
    (every row and every column sums to the number of epochs), below the 99.9 % quantile 296.1."""
    N, epochs = 16, 4000
    counts = np.zeros((N, N))
    pos = np.arange(N)
    for e in range(epochs):
        counts[pos, lr.permute(pos, N, 3, e)] += 1
    expect = epochs / N
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f"chi2 = {chi2:.1f} on 225 degrees of freedom")
    assert chi2 < 296.1


@pytest.mark.parametrize("H,W", [(360, 480), (33, 47), (40, 56), (7, 5)])
def test_boxes_lie_inside_the_frame_and_the_ratio_range(H, W):
    accepted = 0
    for i in range(300):
        top, left, bh, bw, tries, _ = lr.box(H, W, 1, 2, i, i % 3, DRAW)
        assert 1 <= bh <= H and 1 <= bw <= W and 0 <= top <= H - bh and 0 <= left <= W - bw, (i, top, left, bh, bw)
        if tries < 10:
            # bw / bh within the ratio range up to the rounding of both sides: the unrounded sides have exactly a ratio inside
            # it, and each side moves by at most one half
            accepted += 1
            assert (bw - 0.5) / (bh + 0.5) <= DRAW[3] * (1 + 1e-12) and (bw + 0.5) / max(bh - 0.5, 1e-300) >= DRAW[2] * (1 - 1e-12), (i, bh, bw)
    assert accepted > 250


def test_a_frame_no_try_fits_takes_the_fallback():
    """1000 x 10 (H x W): W / H = 0.01 is below every ratio, a box of ratio >= 3/4 and area >= 8 % of the frame is wider than 10."""
    for i in range(200):
        top, left, bh, bw, tries, _ = lr.box(1000, 10, 5, 0, i, 0, DRAW)
        assert tries == 10 and (bw, bh) == (10, 13) and (top, left) == (493, 0), (i, top, left, bh, bw, tries)
    # the wide side: H x W = 6 x 200 -> bh = 6, bw = rint(6 * 4 / 3) = 8, centred; in the range: the whole frame (never with ten
    # tries in practice, so the branch is called on its own draw: a scale range no box can meet)
    assert lr.box(6, 200, 5, 0, 0, 0, DRAW)[:5] == (0, 96, 6, 8, 10)
    assert lr.box(30, 30, 5, 0, 0, 0, lr.draw_params(scale=(4.0, 5.0)))[:5] == (0, 0, 30, 30, 10)


def test_window_starts_cover_their_range():
    starts = [lr.wave_start(9, 1, i, 37) for i in range(2000)]
    assert min(starts) == 0 and max(starts) == 37 and len(set(starts)) == 38
    assert all(lr.wave_start(9, 1, i, 0) == 0 for i in range(50))
    big = [lr.wave_start(9, 1, i, 80000) for i in range(2000)]
    assert 0 <= min(big) < 400 and 79600 < max(big) <= 80000
    assert starts != [lr.wave_start(9, 2, i, 37) for i in range(2000)]  # another epoch, another draw


def test_counters_stay_in_the_loaders_range():
    """Word 1 of every counter has bits 31 and 30 set -- the modulation's are below 2^29, the probabilistic-embedding branch's are
    0x80000000 | modality -- and differs between purposes, frames and tries."""
    seen = set()
    for purpose in (lr.PERM, lr.BOX, lr.FLIP, lr.WAVE):
        for t in (0, 1, 63):
            for k in (0, 5, 9):
                w1 = lr.counter_word1(purpose, t, k)
                assert w1 >> 30 == 3 and w1 < 1 << 32
                seen.add(w1)
    assert len(seen) == 36
    assert lr.words(1, 0, 5, lr.BOX, 0, 0) != lr.words(1, 0, 5, lr.FLIP, 0, 0) != lr.words(1, 1, 5, lr.FLIP, 0, 0)


def test_flips_follow_p():
    flips = [lr.flip(2, 0, i, i % 3, 0.5) for i in range(4000)]
    assert abs(sum(flips) - 2000) < 4 * 0.5 * 4000 ** 0.5  # four standard deviations
    assert not any(lr.flip(2, 0, i, 0, 0.0) for i in range(200)) and all(lr.flip(2, 0, i, 0, 1.0) for i in range(200))


def test_gpu_seeds_have_no_undecided_try():
    """Condition, not tolerance: for every plan the GPU tests compare (the toy layouts, seeds, epochs and ranges of
    loader_ref.TOY_*, and the 64 x 64 frames of the trainer test), no try's rounded sides change when a r and a / r move by
    8 ulp, so the device's exp and sqrt cannot decide a box differently and the GPU comparison is exact for every row."""
    total = fallbacks = frames_seen = 0
    for N, T in lr.TOY_PLANNER_CASES + lr.TOY_LOADER_CASES:
        _, _, labels, clips, frames = lr.toy_layout(N, T)
        for seed in lr.TOY_SEEDS[:1] if N == 1000 else lr.TOY_SEEDS:
            for epoch in lr.TOY_EPOCHS:
                for shuffle in (0, 1):
                    for first, count in lr.toy_ranges(N):
                        p = lr.plan(clips, frames, labels, T, seed, epoch, first, count, shuffle, 1, 37)
                        total += p["undecided"]
                        fallbacks += p["fallbacks"]
                        frames_seen += count * T
    for epoch in lr.TOY_EPOCHS:
        for i in range(8):
            for t in range(2):
                total += lr.box(64, 64, lr.TOY_SEEDS[0], epoch, i, t, DRAW)[5]
    assert total == 0
    assert 0 < fallbacks < frames_seen // 20  # the 200 x 6 samples' frames, and only they


def test_plan_tables():
    """plan() lays the draws out in the stage kernels' row formats; eval mode is file order, whole frames, no flip, and still a
    drawn start; planning a range in two calls equals planning it in one."""
    rng = np.random.default_rng(0)
    N, T = 67, 3
    clips = np.stack([np.arange(N) * 4000, rng.integers(1000, 3000, N), rng.integers(1, 3, N), rng.integers(0, 2, N), np.full(N, 6000)], 1)
    frames = np.stack([np.arange(N * T) * 8000, np.full(N * T, 40), np.full(N * T, 56)], 1).reshape(N, T, 3)
    labels = rng.integers(0, 6, N)
    full = lr.plan(clips, frames, labels, T, 11, 0, 0, N, 1, 1, 37)
    assert np.array_equal(np.sort(full["index"]), np.arange(N)) and np.array_equal(full["label"], labels[full["index"]])
    assert np.array_equal(full["wave_desc"][:, :4], clips[full["index"], :4]) and np.array_equal(full["wave_desc"][:, 5], clips[full["index"], 4])
    assert np.array_equal(full["crop_desc"][:, 0].reshape(N, T), frames[full["index"], :, 0])
    a, b = lr.plan(clips, frames, labels, T, 11, 0, 0, 29, 1, 1, 37), lr.plan(clips, frames, labels, T, 11, 0, 29, N - 29, 1, 1, 37)
    for k in ("index", "label", "wave_desc", "crop_desc"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), full[k]), k
    ev = lr.plan(clips, frames, labels, T, 11, 0, 0, N, 0, 0, 37)
    assert np.array_equal(ev["index"], np.arange(N)) and np.array_equal(ev["crop_desc"][:, 3:], np.tile([0, 0, 40, 56, 0], (N * T, 1)))
    # keyed by the sample, not by the position: the sample's rows are the same in the shuffled and the unshuffled epoch
    un = lr.plan(clips, frames, labels, T, 11, 0, 0, N, 0, 1, 37)
    assert np.array_equal(un["wave_desc"][full["index"]], full["wave_desc"])
    assert np.array_equal(un["crop_desc"].reshape(N, T, 8)[full["index"]], full["crop_desc"].reshape(N, T, 8))
    assert ev["wave_desc"][:, 4].max() > 0 and np.array_equal(ev["wave_desc"], un["wave_desc"])
