"""Time gdl_frames_resized_crop alone on the GPU and the same batch through PyTorch's CPU resize.

A B = 64, T = 3 batch of 360 x 480 uint8 frames (seeded noise), two forms: training (seeded RandomResizedCrop boxes and flips) and
evaluation (whole-frame Resize((224, 224))).  Per form: the launch between device events (warm-up, then --repeats single
launches, median and range; the descriptor table and the frames are on the device before the clock starts; the launches rotate
over --sets copies of the source and output buffers, three by default = 645 MB, so that a launch does not find its 215 MB in the
256 MB Infinity Cache from the launch before), the bytes the algorithm needs -- the boxes' bytes read once plus the float32
output written once -- the rate that gives, and its share of the 6.3 TB/s of HBM bandwidth a kernel can reach on an MI355X.
For comparison the same boxes through F.interpolate(uint8, antialias=True) + flip + normalise on the CPU (a host clock), three
ways: one worker with one thread (what one core does); --workers worker PROCESSES with one thread each, the frames dealt out
among them -- the shape of a DataLoader with that many workers: fresh child processes of this tool that never touch the GPU, all
started on one signal, the batch being done when the slowest has finished its share (threads in one process do not scale: the
per-frame Python between the resizes holds the interpreter lock); and one serial loop over the frames with --workers intra-op
threads, which is NOT that many cores' worth of work (a 360 x 480 frame is too small to split) and is printed to show it.  Needs
a GPU; reads nothing outside the repository.

    python tools/bench_augment.py [--repeats 50] [--workers 16] [--out profiles/augment_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))

from gdl import _lib as L  # noqa: E402
from gdl import data as gd  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s


STEP_FRAMES_PER_S = 39000  # what the B = 64, T = 3 step consumes at 13 000 samples/s (README)


def gpu_times(srcs, desc, n, B, T, size, outs, warmup, repeats):
    m = (ctypes.c_float * 3)(*gd.IMAGENET_MEAN)
    s = (ctypes.c_float * 3)(*gd.IMAGENET_STD)

    def launch(i):
        src, out = srcs[i % len(srcs)], outs[i % len(outs)]
        L.call("gdl_frames_resized_crop", L.ptr(src), src.numel(), L.ptr(desc), n, B, T, size, size, ctypes.cast(m, ctypes.c_void_p),
               ctypes.cast(s, ctypes.c_void_p), L.ptr(out), L.cur_stream())

    for i in range(warmup):
        launch(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(i)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


MEAN = torch.tensor(gd.IMAGENET_MEAN).view(3, 1, 1)
STD = torch.tensor(gd.IMAGENET_STD).view(3, 1, 1)


def cpu_frame(frames, boxes, flips, T, size, out, n):
    t, l, h, w = boxes[n]
    x = frames[n, t:t + h, l:l + w].permute(2, 0, 1)[None]  # channels_last view of the HWC crop, as torchvision makes it
    y = F.interpolate(x, size=(size, size), mode="bilinear", antialias=True)[0]
    if flips[n]:
        y = y.flip(-1)
    out[n // T, :, n % T] = (y.float().div(255.0) - MEAN) / STD


B, T, H, W, SIZE = 64, 3, 360, 480, 224


def make_batch():
    """The seeded batch: frames uint8 [B * T, H, W, 3] on the host and the two forms {name: (boxes, flips)}."""
    n = B * T
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g)
    train_boxes = gd.random_resized_crop_params([(H, W)] * n, generator=g)
    train_flips = gd.random_flips(n, generator=g)
    return frames, {"train (RandomResizedCrop boxes + flips)": (train_boxes, train_flips),
                    "eval (whole-frame Resize)": (torch.tensor([[0, 0, H, W]] * n), torch.zeros(n, dtype=torch.bool))}


def cpu_times(frames, boxes, flips, first, step, threads, repeats, wait=None):
    """Times in ms of frames first, first + step, ... of the batch through the CPU transform, each resize with `threads` intra-op
    threads; one untimed pass first, then wait() if given (the workers' common start)."""
    out = torch.empty(B, 3, T, SIZE, SIZE)
    torch.set_num_threads(threads)

    def share():
        for n in range(first, B * T, step):
            cpu_frame(frames, boxes, flips, T, SIZE, out, n)

    share()
    if wait is not None:
        wait()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        share()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def cpu_worker(k, workers, form, repeats):
    """Child process k of `workers`: its share of the batch, started when the parent says so; prints its times."""
    frames, forms = make_batch()
    boxes, flips = list(forms.values())[form]

    def wait():
        print("ready", flush=True)
        start = float(sys.stdin.readline())
        while time.time() < start:
            time.sleep(0.0005)

    print(" ".join(f"{v:.3f}" for v in cpu_times(frames, boxes.tolist(), flips.tolist(), k, workers, 1, repeats, wait)), flush=True)


def cpu_workers(workers, form, repeats):
    """`workers` child processes, one thread each, frame n to worker n % workers.  Returns per repeat the time of the slowest
    worker (they start together and run the same number of repeats, so repeat r of all workers overlaps)."""
    ps = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", str(k), "--workers", str(workers), "--form", str(form),
                            "--cpu-repeats", str(repeats)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True) for k in range(workers)]
    try:
        for p in ps:
            if p.stdout.readline().strip() != "ready":
                raise RuntimeError("bench_augment: a CPU worker did not start")
        start = time.time() + 0.5
        for p in ps:
            p.stdin.write(f"{start!r}\n")
            p.stdin.flush()
        per = [[float(v) for v in p.stdout.readline().split()] for p in ps]
    finally:
        for p in ps:
            p.stdin.close()
            p.wait(timeout=60)
    return [max(w[r] for w in per) for r in range(repeats)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workers", type=int, default=16, help="CPU workers of the host comparison (a GPU job gets 16 cores)")
    ap.add_argument("--sets", type=int, default=3, help="copies of the source / output buffers the timed launches rotate over")
    ap.add_argument("--cpu-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu-worker", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--form", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--commit", default=None, help="what to print as the commit (default: git rev-parse of the repository)")
    a = ap.parse_args()
    if a.cpu_worker is not None:
        return cpu_worker(a.cpu_worker, a.workers, a.form, a.cpu_repeats)
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: no GPU visible; nothing is measured without one")
    n, size = B * T, SIZE
    frames, forms = make_batch()
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = [f"bench_augment: B {B}, T {T}, {H} x {W} uint8 sources -> {size} x {size} float32, {torch.cuda.get_device_name(0)}, "
             f"torch {torch.__version__}, commit {commit or 'unknown (no git here)'}",
             f"GPU: one gdl_frames_resized_crop launch between device events, {a.warmup} warm-up, {a.repeats} repeats, rotating over "
             f"{a.sets} sets of source + output buffers ({a.sets * (n * H * W * 3 + 4 * 3 * n * size * size) / 1e6:.0f} MB; Infinity Cache 256 MB)",
             f"CPU: F.interpolate(uint8, antialias=True) per frame + flip + normalise, {a.cpu_repeats} repeats of the batch; the step "
             f"consumes {STEP_FRAMES_PER_S} frames/s"]
    srcs = [frames.cuda() for _ in range(a.sets)]
    outs = [torch.empty(B, 3, T, size, size, device="cuda") for _ in range(a.sets)]
    for name, (boxes, flips) in forms.items():
        desc, _, _ = gd.crop_descriptors([(H, W)] * n, boxes, flips, T, size)
        ms = gpu_times(srcs, desc.cuda(), n, B, T, size, outs, a.warmup, a.repeats)
        read = int((boxes[:, 2] * boxes[:, 3]).sum()) * 3
        written = 4 * 3 * n * size * size
        med = statistics.median(ms)
        rate = (read + written) / (med * 1e-3)
        bl, fl = boxes.tolist(), flips.tolist()
        lines += [f"{name}:",
                  f"  bytes: {read / 1e6:.1f} MB of boxes read + {written / 1e6:.1f} MB written = {(read + written) / 1e6:.1f} MB",
                  f"  GPU launch: median {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}) -> {rate / 1e9:.0f} GB/s, "
                  f"{100 * rate / HBM_ACHIEVABLE:.1f} % of 6.3 TB/s; {n / (med * 1e-3):.0f} frames/s"]
        k = list(forms).index(name)
        for label, ms_cpu in ((f"1 worker x 1 thread (one core)", cpu_times(frames, bl, fl, 0, 1, 1, a.cpu_repeats)),
                              (f"{a.workers} worker processes x 1 thread (frames dealt out; slowest worker)", cpu_workers(a.workers, k, a.cpu_repeats)),
                              (f"1 serial loop, {a.workers} intra-op threads (not {a.workers} cores of work)",
                               cpu_times(frames, bl, fl, 0, 1, a.workers, a.cpu_repeats))):
            cmed = statistics.median(ms_cpu)
            fps = n / (cmed * 1e-3)
            lines.append(f"  CPU, {label}: median {cmed:.1f} ms (min {min(ms_cpu):.1f}, max {max(ms_cpu):.1f}) -> {fps:.0f} frames/s = "
                         f"{fps / STEP_FRAMES_PER_S:.2f} of what the step consumes; GPU launch {cmed / med:.0f}x faster")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
