"""A NumPy restatement of gdl_loader_plan (include/gdl_hip.h): the epoch order, the window starts, the crop boxes and the flips
of the device-resident loader as functions of (seed, epoch, sample index), on modulation_ref.philox4x32_10.  Plain loops over
positions and frames; the integers are Python's, the floating point is IEEE double in the order the header spells.

plan() also reports, per try of a crop box, whether the try is *decided*: the rounded sides rint(sqrt(a r)), rint(sqrt(a / r))
are the same when a r and a / r are each moved by +-8 ulp.  The device's exp and sqrt may differ from NumPy's by a few ulp (the
products, sums and quotients around them are the same IEEE operations on both sides, nothing is fused), and a try whose rounding
survives 8 ulp either way cannot come out differently there.  With zero undecided tries the device's tables equal these exactly."""
import math

import numpy as np

from modulation_ref import philox4x32_10

PERM, BOX, FLIP, WAVE = 0, 1, 2, 3
DEFAULT_SCALE, DEFAULT_RATIO, DEFAULT_P_FLIP = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0), 0.5
ULPS = 8


def draw_params(scale=DEFAULT_SCALE, ratio=DEFAULT_RATIO, p_flip=DEFAULT_P_FLIP):
    """The seven doubles of gdl_loader_plan's `draw`; the logarithms are math.log's, as gdl.loader takes them."""
    return [float(scale[0]), float(scale[1]), float(ratio[0]), float(ratio[1]), math.log(float(ratio[0])), math.log(float(ratio[1])),
            float(p_flip)]


def counter_word1(purpose, t, k):
    return 0xC0000000 | purpose << 24 | t << 8 | k


def words(seed, epoch, c0, purpose, t=0, k=0):
    """The four words of one counter, as Python ints.  c0 may be an array: then four uint32 arrays."""
    seed, epoch = int(seed) & (1 << 64) - 1, int(epoch) & (1 << 64) - 1
    w = philox4x32_10((c0, counter_word1(purpose, t, k), epoch & 0xFFFFFFFF, epoch >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return tuple(int(x) for x in w) if np.ndim(c0) == 0 else w


def u(w):
    return (float(w) + 0.5) * 2.0 ** -32


def kbits(N):
    return max(1, -(-(int(N) - 1).bit_length() // 2))


def permute(pos, N, seed, epoch, passes=None):
    """The keyed bijection of [0, N), vectorised over an array of positions.  passes: a list that receives the longest walk."""
    N = int(N)
    kb = kbits(N)
    mask = (1 << kb) - 1
    v = np.array(pos, dtype=np.uint64).reshape(-1)
    out = np.empty_like(v)
    todo = np.arange(v.size)
    n = 0
    while todo.size:
        n += 1
        L, R = v >> np.uint64(kb), v & np.uint64(mask)
        for r in range(6):
            f = words(seed, epoch, R, PERM, 0, r)[0].astype(np.uint64) & np.uint64(mask)
            L, R = R, L ^ f
        v = L << np.uint64(kb) | R
        done = v < N
        out[todo[done]] = v[done]
        todo, v = todo[~done], v[~done]
    if passes is not None:
        passes.append(n)
    return out.astype(np.int64).reshape(np.shape(pos))


def _moved(x, ulps):
    y = np.float64(x)
    for _ in range(abs(ulps)):
        y = np.nextafter(y, np.inf if ulps > 0 else -np.inf)
    return y


def _side(x):
    return float(np.rint(np.sqrt(np.float64(x))))


def box(H, W, seed, epoch, index, t, draw):
    """-> (top, left, bh, bw, tries, undecided): the box of frame t of sample `index`; tries = 10 if the fallback was taken."""
    s_lo, s_hi, r_lo, r_hi, lr_lo, lr_hi, _ = draw
    H, W = int(H), int(W)
    area = float(H * W)
    undecided = 0
    for k in range(10):
        w = words(seed, epoch, index, BOX, t, k)
        a = area * (s_lo + (s_hi - s_lo) * u(w[0]))
        r = float(np.exp(np.float64(lr_lo + (lr_hi - lr_lo) * u(w[1]))))
        ar, aq = a * r, a / r
        cw, ch = _side(ar), _side(aq)
        if not (cw == _side(_moved(ar, ULPS)) == _side(_moved(ar, -ULPS)) and ch == _side(_moved(aq, ULPS)) == _side(_moved(aq, -ULPS))):
            undecided += 1
        if 0 < cw <= W and 0 < ch <= H:
            bw, bh = int(cw), int(ch)
            return (w[2] * (H - bh + 1)) >> 32, (w[3] * (W - bw + 1)) >> 32, bh, bw, k, undecided
    in_ratio = float(W) / float(H)
    bh, bw = H, W
    if in_ratio < r_lo:
        bh = min(H, max(1, int(np.rint(np.float64(W) / np.float64(r_lo)))))
    elif in_ratio > r_hi:
        bw = min(W, max(1, int(np.rint(np.float64(H) * np.float64(r_hi)))))
    return (H - bh) // 2, (W - bw) // 2, bh, bw, 10, undecided


def flip(seed, epoch, index, t, p_flip):
    return int(u(words(seed, epoch, index, FLIP, t, 0)[0]) < p_flip)


def wave_start(seed, epoch, index, start_high):
    return (words(seed, epoch, index, WAVE, 0, 0)[0] * (int(start_high) + 1)) >> 32


def plan(clips, frames, labels, T, seed, epoch, first, count, shuffle, augment, start_high, draw=None):
    """clips [N][5], frames [N][T][3], labels [N] (integer arrays) -> dict(index [count], label [count], wave_desc [count][6],
    crop_desc [count * T][8], undecided: the number of undecided tries, fallbacks: the number of frames on the fallback)."""
    draw = draw_params() if draw is None else draw
    clips, frames, labels = (np.asarray(a, dtype=np.int64) for a in (clips, frames, labels))
    N = labels.shape[0]
    frames = frames.reshape(N, T, 3)
    pos = np.arange(first, first + count, dtype=np.int64)
    index = permute(pos, N, seed, epoch) if shuffle else pos.copy()
    wave_desc = np.empty((count, 6), dtype=np.int64)
    crop_desc = np.empty((count * T, 8), dtype=np.int64)
    undecided = fallbacks = 0
    for p, i in enumerate(index.tolist()):
        wave_desc[p] = [*clips[i, :4], wave_start(seed, epoch, i, start_high), clips[i, 4]]
        for t in range(T):
            off, H, W = frames[i, t].tolist()
            if augment:
                top, left, bh, bw, tries, und = box(H, W, seed, epoch, i, t, draw)
                undecided += und
                fallbacks += tries == 10
                fl = flip(seed, epoch, i, t, draw[6])
            else:
                top, left, bh, bw, fl = 0, 0, H, W, 0
            crop_desc[p * T + t] = [off, H, W, top, left, bh, bw, fl]
    return dict(index=index, label=labels[index], wave_desc=wave_desc, crop_desc=crop_desc, undecided=undecided, fallbacks=fallbacks)


# ---------------------------------------------------------------- the toy dataset of test_loader_cpu.py / test_loader_gpu.py
TOY_AUDIO = dict(rate=16000, n_samples=1000, tiling=("double", 1100), start_high=37, n_fft=64, hop_length=16, resize=None)
TOY_SIZE = 32
TOY_SEEDS, TOY_EPOCHS = (11, 12), (0, 3)


def toy_layout(N, T):
    """Shapes only: int16 stereo and float32 mono clips of ragged length, frames of 40 x 56 and 33 x 47 mixed (also within a
    sample; 33 * 47 * 3 bytes is no whole number of dwords), one 200 x 6 sample that no try fits.  -> (clip_meta [(len, channels,
    format)], sizes [N][T] of (H, W), labels [N], clips [N][5], frames [N][T][3]) with the tables as gdl.DeviceDataset lays
    them out: every clip and frame on a dword, limit by the toy's doubling rule."""
    rng = np.random.default_rng(1000 * N + T)
    lengths = rng.integers(300, 1500, N)
    meta = [(int(n), 2, 1) if i % 2 == 0 else (int(n), 1, 0) for i, n in enumerate(lengths)]  # format 1 = int16, 0 = float32
    sizes = [[(200, 6) if i == N // 2 else ((40, 56), (33, 47))[(i + t) % 2] for t in range(T)] for i in range(N)]
    labels = rng.integers(0, 6, N)
    clips, off = [], 0
    for n, ch, fmt in meta:
        limit = n
        while limit < TOY_AUDIO["tiling"][1]:
            limit *= 2
        clips.append([off, n, ch, fmt, limit])
        off += (n * ch * (2 if fmt else 4) + 3) // 4 * 4
    frames, off = [], 0
    for per_sample in sizes:
        for h, w in per_sample:
            frames.append([off, h, w])
            off += (h * w * 3 + 3) // 4 * 4
    return meta, sizes, labels.astype(np.int64), np.array(clips, dtype=np.int64), np.array(frames, dtype=np.int64).reshape(N, T, 3)


# the (N, T) the GPU planner test walks, the ranges of positions it plans at each N (first, count: cut at odd places), and the
# datasets of the loader tests; test_loader_cpu.py checks that none of these holds an undecided try
TOY_PLANNER_CASES = [(N, T) for N in (1, 2, 5, 67, 1000) for T in (1, 3)]
TOY_LOADER_CASES = [(13, 3), (67, 1)]


def toy_ranges(N):
    return [(0, N)] if N <= 67 else [(0, 77), (333, 150), (N - 61, 61)]
