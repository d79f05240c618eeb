"""Time the device-resident epoch loader (gdl.DeviceDataset / gdl.DeviceLoader over gdl_loader_plan) on synthetic data at the
CREMA-D frame shapes (B = 64, T = 3, 360 x 480 frames -> 224 x 224) with the Kinetics-Sounds audio stage (int16 stereo clips of
10 s at 16 kHz, a 5 s window at a drawn start, n_fft 256 / hop 128), and the path it replaces.

  (a) the planning launch, gdl_loader_plan for a whole epoch (shuffle and augmentation on), between device events, at N = 6 400
      and N = 2^17 samples (tables only: the planner reads no pixel and no sample);
  (b) host time per batch on the step's own thread: next(loader) against today's path for the same batch --
      random_augment_params + resized_crop_frames + stage_audio with host draws (gdl.data) -- each as the host clock of the call
      alone (what the thread is busy for: the launches are asynchronous) and as the host clock ending in a device synchronise;
  (c) the trainer loop: --steps DGLTrainer.step calls (Kinetics-Sounds model, bf16) fed by the loader, without and with stream=,
      beside the same steps on one fixed pre-staged batch, as time per step between a synchronise before and after the loop;
      the difference to the fixed batch is what the loader costs in the loop;
  (d) with --parent DIR: bench.py's own step in this tree and in DIR, a checkout of the parent commit with its library built
      (the binding loads every symbol of its own header, so a library goes with its tree), child processes taken in turn
      before this process touches the device.
Every figure is the median of --rounds rounds that take the variants in turn, with the lowest and highest round in brackets.
Needs a GPU; reads nothing outside the repository.

    python tools/bench_loader.py [--rounds 5] [--samples 1600] [--steps 100] [--parent DIR] [--out profiles/loader_bench.txt]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))

B, T, H, W, SIZE, CLIP_LEN = 64, 3, 360, 480, 224, 160000
AUDIO = "KineticSound"


def fig(rounds, unit="ms"):
    return f"{statistics.median(rounds):.4f} {unit} ({min(rounds):.4f} .. {max(rounds):.4f})"


def bench_py(tree, steps, warmup):
    env = dict(os.environ)
    env.pop("GDL_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       env=env, capture_output=True, text=True, timeout=900, cwd=tree)
    if r.returncode != 0:
        raise SystemExit(f"bench_loader: {tree}/bench.py failed ({r.returncode}): {r.stderr[-1500:]}")
    ms = json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]
    print(f"bench_loader: bench.py of {tree}: {ms} ms/step", file=sys.stderr, flush=True)
    return ms


def part_d(a):
    ours, parent = [], []
    for _ in range(a.bench_rounds):
        ours.append(bench_py(ROOT, a.steps, 20))
        parent.append(bench_py(os.path.abspath(a.parent), a.steps, 20))
    d = statistics.median(ours) - statistics.median(parent)
    spread = max(max(ours) - min(ours), max(parent) - min(parent))
    return [f"(d) bench.py --gpus 1 --steps {a.steps} --warmup 20, {a.bench_rounds} child processes each, taken in turn:",
            f"    this build:    {fig(ours, 'ms/step')}",
            f"    parent commit: {fig(parent, 'ms/step')}",
            f"    difference of the medians {d:+.4f} ms, run-to-run spread {spread:.4f} ms: "
            + ("unchanged within the spread" if abs(d) <= spread else "OUTSIDE the spread")]


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


def part_a(a, L):
    lines = ["(a) gdl_loader_plan, one launch for a whole epoch (shuffle = augment = 1, T = 3, 360 x 480 frames), device events, "
             f"median of {a.repeats} launches per round:"]
    draw = (ctypes.c_double * 7)(0.08, 1.0, 0.75, 4.0 / 3.0, math.log(0.75), math.log(4.0 / 3.0), 0.5)
    for N in (6400, 1 << 17):
        i = torch.arange(N, dtype=torch.int64)
        clips = torch.stack([i * (CLIP_LEN * 4), torch.full_like(i, CLIP_LEN), torch.full_like(i, 2), torch.ones_like(i),
                             torch.full_like(i, CLIP_LEN)], 1).cuda()
        j = torch.arange(N * T, dtype=torch.int64)
        frames = torch.stack([j * (H * W * 3), torch.full_like(j, H), torch.full_like(j, W)], 1).cuda()
        labels = (i % 34).cuda()
        out = [torch.empty(N * w, dtype=torch.int64, device="cuda") for w in (1, 1, 6, 8 * T)]
        epoch = [0]

        def launch():
            epoch[0] += 1
            L.call("gdl_loader_plan", L.ptr(clips), L.ptr(frames), L.ptr(labels), N, T, 0, epoch[0], 0, N, 1, 1, 80000, 80000, SIZE, SIZE,
                   ctypes.cast(draw, ctypes.c_void_p), *[L.ptr(o) for o in out], L.cur_stream())

        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        assert sorted(out[0].tolist()) == list(range(N))
        rounds = [events(launch, a.repeats) for _ in range(a.rounds)]
        mb = sum(o.numel() for o in out) * 8 / 1e6
        lines.append(f"    N = {N:6d}: {fig(rounds)}; {mb:.1f} MB of tables written, {N * T} boxes drawn")
    return lines


def make_dataset(a):
    import gdl

    g = torch.Generator(device="cuda").manual_seed(0)
    N = a.samples
    frames = torch.randint(0, 256, (N, T, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    clips = [torch.randint(-32768, 32768, (CLIP_LEN, 2), generator=g, device="cuda", dtype=torch.int32).to(torch.int16) for _ in range(N)]
    labels = torch.randint(0, 34, (N,), generator=g, device="cuda").cpu()
    return gdl.DeviceDataset(clips, frames, labels, AUDIO, T, size=SIZE), frames, clips


def part_b(a, ds, frames, clips):
    import gdl
    from gdl import data as gd

    loader = gdl.DeviceLoader(ds, B, True, seed=0)
    n_batches = len(loader)
    packed, meta = gd.pack_clips(clips[:B])
    desc = gd.wave_descriptors(meta, [0] * B, [gd.wave_limit(CLIP_LEN, gd.AUDIO_STAGES[AUDIO]["tiling"])] * B,
                               gd.AUDIO_STAGES[AUDIO]["n_samples"])[0]
    batch_frames = frames[:B].reshape(B * T, H, W, 3)
    sizes = [(H, W)] * (B * T)
    image = torch.empty(B, 3, T, SIZE, SIZE, device="cuda")
    spec = torch.empty(B, 129, 626, device="cuda")
    gen = torch.Generator().manual_seed(0)

    def today():
        boxes, flips = gd.random_augment_params(sizes, generator=gen)
        gd.resized_crop_frames(batch_frames, boxes, flips, SIZE, T=T, out=image)
        gd.stage_audio((packed, desc), AUDIO, generator=gen, out=spec)

    def run(fn, n, sync_each):
        """Median host time of a call: the call alone (the device drained before it, not after), or ending in a synchronise."""
        ms = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if sync_each:
                torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        return statistics.median(ms)

    state = {"it": None}

    def next_batch():
        try:
            return next(state["it"])
        except (StopIteration, TypeError):
            state["it"] = iter(loader)  # a new pass over the epoch: one planning launch, then the first batch
            return next(state["it"])

    n = min(a.repeats, n_batches - 1)
    r = {k: [] for k in ("next", "next_sync", "today", "today_sync")}
    for fn in (today, next_batch):
        for _ in range(3):
            fn()
    for _ in range(a.rounds):
        r["next"].append(run(next_batch, n, False))
        r["today"].append(run(today, max(5, n // 4), False))
        r["next_sync"].append(run(next_batch, n, True))
        r["today_sync"].append(run(today, max(5, n // 4), True))
    return [f"(b) host time per batch of B = {B} on the calling thread (N = {ds.N}, {ds.nbytes / 1e9:.2f} GB on the device; a pass over "
            f"the epoch is {n_batches} batches, its planning launch falls into the first next()):",
            f"    next(loader), the call alone:                                   {fig(r['next'])}",
            f"    random_augment_params + resized_crop_frames + stage_audio, alone: {fig(r['today'])}",
            f"    next(loader) + synchronise:                                     {fig(r['next_sync'])}",
            f"    today's path + synchronise:                                     {fig(r['today_sync'])}",
            f"    today's path over next(loader), calls alone: {statistics.median(r['today']) / statistics.median(r['next']):.0f}x"]


def part_c(a, ds):
    import bench
    import gdl
    from gdl.trainer import DGLTrainer

    wl = bench.WORKLOADS["ks"]
    model, _ = bench.build_model(wl, B, torch.device("cuda", 0))
    tr = DGLTrainer(model, lr=2e-3, alpha=wl["alpha"], momentum=0.9, weight_decay=1e-4, max_norm=40.0, dtype="bf16")
    side = torch.cuda.Stream()
    loaders = {"loader": gdl.DeviceLoader(ds, B, True, seed=0), "loader, stream=": gdl.DeviceLoader(ds, B, True, seed=0, stream=side)}
    fixed = tuple(t.clone() for t in next(iter(loaders["loader"])))

    def fed(ld):
        def run(steps):
            done, epoch = 0, 0
            while done < steps:
                ld.set_epoch(epoch)
                for spec, image, label in ld:
                    tr.step(spec, image, label)
                    done += 1
                    if done == steps:
                        break
                epoch += 1
        return run

    def fixed_batch(steps):
        for _ in range(steps):
            tr.step(*fixed)

    variants = {"fixed pre-staged batch": fixed_batch, **{k: fed(v) for k, v in loaders.items()}}
    for fn in variants.values():
        fn(15)
    torch.cuda.synchronize()
    r = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(a.steps)
            torch.cuda.synchronize()
            r[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    base = statistics.median(r["fixed pre-staged batch"])
    spread = max(max(v) - min(v) for v in r.values())
    lines = [f"(c) {a.steps} DGLTrainer.step calls (Kinetics-Sounds model, bf16, B = {B}), time per step from a synchronise before the "
             f"loop to one after it ({math.ceil(a.steps / len(loaders['loader']))} epochs of {len(loaders['loader'])} batches, their "
             "planning launches included):"]
    for k, v in r.items():
        lines.append(f"    {k + ':':26s} {fig(v, 'ms/step')}" + ("" if k.startswith("fixed") else f"   {statistics.median(v) - base:+.4f} ms against the fixed batch"))
    d = statistics.median(r["loader, stream="]) - statistics.median(r["loader"])
    lines.append(f"    stream= against the plain loader: {d:+.4f} ms per step; largest run-to-run spread of a variant {spread:.4f} ms: "
                 + ("the side stream's effect is not resolved" if abs(d) <= spread else
                    "the side stream pays" if d < 0 else "the side stream does not pay"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20, help="calls per round in (a) and (b)")
    ap.add_argument("--samples", type=int, default=1600, help="samples of the synthetic dataset of (b) and (c)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--parent", default=None, help="(d): a checkout of the parent commit, built")
    ap.add_argument("--bench-rounds", type=int, default=3, help="(d): bench.py child processes per build")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to print as the commit (default: git rev-parse of the repository)")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if a.samples < 4 * B:
        ap.error(f"--samples must be at least {4 * B}")
    lines_d = part_d(a) if a.parent else ["(d) bench.py beside the parent commit: not measured in this run (no --parent)"]
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader: no GPU visible; nothing is measured without one")
    from gdl import _lib as L

    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = [f"bench_loader: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, commit {commit or 'unknown (no git here)'}; "
             f"{a.rounds} rounds that take the variants in turn; a figure is the median of the rounds, in brackets the lowest and highest round"]
    lines += part_a(a, L)
    ds, frames, clips = make_dataset(a)
    lines += part_b(a, ds, frames, clips)
    del frames, clips
    lines += part_c(a, ds)
    lines += lines_d
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
