"""Time gdl_wave_logspec -- waveform staging + log spectrogram in one launch from device-resident clips -- against what it
replaces: the NumPy staging of the same batch on the host, its host-to-device copy and gdl_logspec on the staged batch.

Two seeded batches of B = 64: the CREMA-D shape (float32 mono clips of 1.3 to 5 s at 22050 Hz, three copies, the first 3 s,
n_fft 512 / hop 353) and the Kinetics-Sounds shape (int16 stereo clips of 10 s at 16 kHz, a 5 s window at a drawn start, 256 / 128).
Per batch, in --rounds rounds that take the measurements in turn (so that a drift of the machine shows as spread and not as a
difference), --repeats single calls each:
  (1)  the gdl_wave_logspec launch between device events, clips and descriptor table on the device;
  (1s) the same as a caller's step: gd.wave_log_spectrogram((packed, desc), starts) -- window check, table upload, launch -- on a host
       clock that ends in a device synchronise;
  (2)  gdl_logspec alone on the pre-staged float32 batch, between device events: (1) - (2) is what the loader costs;
  (3)  the NumPy staging of the batch (per sample: / 32768, np.mean, np.tile, slice, clip; np.stack) plus torch's copy of the
       staged batch to the device, host clock ending in a synchronise: what the stage replaces.
A figure is the median of its round medians, with the lowest and highest round median as the run-to-run spread.  The outputs of
(1) and (2) are compared bit for bit before anything is timed.  A launch's working set is smaller than the 256 MB Infinity Cache
and the launches follow each other directly, so (1) and (2) are warm-cache figures.  Needs a GPU; reads nothing outside the
repository.

    python tools/bench_wave.py [--rounds 5] [--repeats 40] [--out profiles/wave_bench.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))

from gdl import _lib as L  # noqa: E402
from gdl import data as gd  # noqa: E402

B = 64


def make_batch(name):
    """Seeded clips as the files hold them (NumPy, on the host) and the starts of one step."""
    st = gd.AUDIO_STAGES[name]
    rng = np.random.default_rng(0)
    if name == "CREMAD":
        lengths = rng.integers(int(1.3 * 22050), 5 * 22050 + 1, B)
        clips = [(rng.standard_normal(int(n)) * 0.4).astype(np.float32) for n in lengths]
    else:
        clips = [rng.integers(-32768, 32768, (160000, 2)).astype(np.int16) for _ in range(B)]
    starts = gd.random_wave_starts(B, st["start_high"], torch.Generator().manual_seed(0)).tolist()
    return st, clips, starts


def numpy_stage(clips, starts, st):
    """The datasets' host code for one batch (tests/wave_ref.py has the same lines)."""
    rows = []
    for raw, start in zip(clips, starts):
        x = raw.astype(np.float32) / np.float32(32768.0) if raw.dtype == np.int16 else raw
        x = np.mean(x, axis=1, dtype=np.float32) if x.ndim == 2 else x
        kind, arg = st["tiling"]
        if kind == "times":
            x = np.tile(x, arg)
        else:
            while len(x) < arg:
                x = np.tile(x, 2)
        w = x[start:start + st["n_samples"]].copy()
        w[w > 1.] = 1.
        w[w < -1.] = -1.
        rows.append(w)
    return np.stack(rows)


def events(fn, repeats):
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def host_clock(fn, repeats):
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def fig(rounds):
    return f"{statistics.median(rounds):.4f} ms (round medians {min(rounds):.4f} .. {max(rounds):.4f})"


def bench(name, a):
    st, clips, starts = make_batch(name)
    n, n_fft, hop = st["n_samples"], st["n_fft"], st["hop_length"]
    limits = [gd.wave_limit(len(c), st["tiling"]) for c in clips]
    packed, meta = gd.pack_clips([torch.from_numpy(c).cuda() for c in clips])
    desc, nbytes = gd.wave_descriptors(meta, starts, limits, n)
    desc_dev = desc.cuda()
    frames = L.load().gdl_logspec_frames(n, hop)
    out = torch.empty(B, n_fft // 2 + 1, frames, device="cuda")
    out2 = torch.empty_like(out)
    staged_np = numpy_stage(clips, starts, st)
    staged = torch.from_numpy(staged_np).cuda()

    def launch():
        L.call("gdl_wave_logspec", L.ptr(packed), packed.numel(), L.ptr(desc_dev), B, n, n_fft, hop, 0, 0, 0, None, L.ptr(out),
               L.cur_stream())

    def step():
        gd.wave_log_spectrogram((packed, desc), n, starts, None, n_fft, hop, out=out)

    def logspec():
        L.call("gdl_logspec", L.ptr(staged), B, n, n_fft, hop, 0, L.ptr(out2), L.cur_stream())

    def host():
        return torch.from_numpy(numpy_stage(clips, starts, st)).cuda()

    launch()
    logspec()
    torch.cuda.synchronize()
    same = torch.equal(out, out2)
    wave = gd.wave_log_spectrogram((packed, desc_dev), n, None, None, n_fft, hop, return_wave=True)[1]
    same_wave = torch.equal(wave, staged)
    for fn in (launch, step, logspec):
        for _ in range(a.warmup):
            fn()
    host()
    torch.cuda.synchronize()
    r = {"launch": [], "step": [], "logspec": [], "host": []}
    for _ in range(a.rounds):
        r["launch"].append(events(launch, a.repeats))
        r["logspec"].append(events(logspec, a.repeats))
        r["step"].append(host_clock(step, a.repeats))
        r["host"].append(host_clock(host, a.host_repeats))
    diff = [x - y for x, y in zip(r["launch"], r["logspec"])]
    spread = max(max(r["launch"]) - min(r["launch"]), max(r["logspec"]) - min(r["logspec"]))
    d = statistics.median(diff)
    verdict = (f"inside the run-to-run spread of {spread:.4f} ms: the loader's cost is not resolved" if abs(d) <= spread else
               f"outside the run-to-run spread of {spread:.4f} ms")
    src_mb, stg_mb, out_mb = nbytes / 1e6, staged.numel() * 4 / 1e6, out.numel() * 4 / 1e6
    return [f"{name}: B {B}, clips {min(len(c) for c in clips)} .. {max(len(c) for c in clips)} samples of {clips[0].dtype}"
            f"{' stereo' if clips[0].ndim == 2 else ' mono'} ({src_mb:.1f} MB packed), window {n}, n_fft {n_fft}, hop {hop} -> "
            f"[{B}, {n_fft // 2 + 1}, {frames}] ({out_mb:.1f} MB); staged batch {stg_mb:.1f} MB",
            f"  outputs: spectrogram of (1) == (2) bit for bit: {same}; wave_out == NumPy staging bit for bit: {same_wave}",
            f"  (1)  gdl_wave_logspec launch, device events:            {fig(r['launch'])}",
            f"  (2)  gdl_logspec on the pre-staged batch, device events: {fig(r['logspec'])}",
            f"  (1) - (2), per round:                                    {d:+.4f} ms ({min(diff):+.4f} .. {max(diff):+.4f}), {verdict}",
            f"  (1s) wave_log_spectrogram((packed, desc), starts), host clock + synchronise: {fig(r['step'])}",
            f"  (3)  NumPy staging + host-to-device copy of the staged batch, host clock:     {fig(r['host'])}",
            f"  (3) + (2) over (1s): {(statistics.median(r['host']) + statistics.median(r['logspec'])) / statistics.median(r['step']):.1f}x"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to print as the commit (default: git rev-parse of the repository)")
    a = ap.parse_args()
    if a.rounds < 3 or a.repeats < 20:
        ap.error("--rounds must be at least 3 and --repeats at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_wave: no GPU visible; nothing is measured without one")
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = [f"bench_wave: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, commit {commit or 'unknown (no git here)'}; "
             f"{a.rounds} rounds x {a.repeats} calls ({a.host_repeats} for the host staging), {a.warmup} warm-up; a figure is the median of the "
             "round medians, in brackets the lowest and highest round median"]
    for name in ("CREMAD", "KineticSound"):
        lines += bench(name, a)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
