#!/usr/bin/env python3
"""The MMPareto step (DGLTrainer(pareto=True)) beside the plain multi-task step it sits on, gdl_pareto_integrate alone at the two
encoders' sizes, and -- the switch off -- the bench.py step of this tree beside another tree's (the parent commit's), on one MI355X.

    python tools/bench_pareto.py [--rounds 5] [--steps 100] [--warmup 20] [--parent DIR] [--out profiles/pareto_bench.txt]

CREMA-D shapes (spec 257 x 188, 3 frames of 224 x 224), B = 64, bf16 encoders, concat head, synthetic batches, one job.
  1. steps: two trainers live in the process and are timed alternately -- per round and trainer `warmup` untimed and `steps` timed
     steps between two device synchronisations (host clock).  Median and lowest .. highest over the rounds.
       mtl concat      detach_fused=False, drop_head_uni=False: loss_f + alpha (loss_a + loss_v), one backward per encoder
       pareto concat   the same with pareto=True: two backwards per encoder and one gdl_pareto_integrate
  2. gdl_pareto_integrate alone on vectors of the audio and the visual encoder's element counts (offset by one float from a 16-byte
     boundary, as a range of the arena is): `launches` back-to-back calls between two device events, `repeats` times; us per call
     and the rate its 20 n bytes (g_m and g_u read twice, g_m written once) correspond to.  The calls rotate over four pairs of
     vectors (4 x 89 MB: more than the 256 MB Infinity Cache, so a call finds its pair evicted, as inside the step), every pair
     restored from a master copy before each timed window (the call works in place).
  3. with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1` in this tree and in DIR as fresh child
     processes, alternating, `bench_rounds` times each; ms_per_step of their result lines.  The pareto switch is off in both.
Nothing here asserts a threshold: the file states what was measured.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-gdl_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gdl.trainer import DGLTrainer  # noqa: E402


def build(fusion, wl, batch, dev):
    """The model as main_dgl.py:230-246 builds it (seeded weight_init)."""
    from models.basic_model import AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    setup_seed(0)
    model = AVClassifier_DGL(argparse.Namespace(fusion_method=fusion, dataset=wl["dataset"], modality="full", batch_size=batch))
    model.apply(weight_init)
    return model.to(dev).train()


def spread(v):
    return f"{float(np.median(v)):.3f}  ({min(v):.3f} .. {max(v):.3f})"


def bench_steps(a, dev, lines):
    wl, B = bench.WORKLOADS["cremad"], a.batch
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]
    mtl = dict(lr=2e-3, max_norm=40.0, dtype="bf16", alpha=2.5, detach_fused=False, drop_head_uni=False)
    trainers = {"mtl concat": DGLTrainer(build("concat", wl, B, dev), **mtl),
                "pareto concat": DGLTrainer(build("concat", wl, B, dev), pareto=True, **mtl)}
    rounds = {k: [] for k in trainers}
    host = {k: [] for k in trainers}
    i = 0
    for _ in range(a.rounds):
        for kind, tr in trainers.items():
            for _ in range(a.warmup):
                tr.step(*data[i % 4])
                i += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step(*data[i % 4])
                i += 1
            torch.cuda.synchronize()
            rounds[kind].append((time.perf_counter() - t0) / a.steps * 1e3)
            for _ in range(10):  # the host's part alone: one step enqueued on an idle device, the call's return taken
                t0 = time.perf_counter()
                tr.step(*data[i % 4])
                host[kind].append((time.perf_counter() - t0) * 1e3)
                i += 1
                torch.cuda.synchronize()
    marks = ("start", "fwd_done", "head_done", "bwd_done", "end")
    phases = {}
    for kind, tr in trainers.items():  # the step's phases on its main stream (device events at DGLTrainer's marks), 20 steps
        tr.phase_events = []
        for _ in range(20):
            tr.step(*data[i % 4])
            i += 1
        torch.cuda.synchronize()
        ev, tr.phase_events = tr.phase_events, None
        assert [n for n, _ in ev[:5]] == list(marks), [n for n, _ in ev[:5]]
        per = np.array([[ev[5 * k + j][1].elapsed_time(ev[5 * k + j + 1][1]) for j in range(4)] for k in range(20)])
        phases[kind] = np.median(per, axis=0)
    chains = {}
    for kind, tr in trainers.items():  # each backward call's begin and end on its own chain's stream (as tools/chain_timeline.py)
        rec = []

        def wrap(fn, name):
            def inner(*args, **kw):
                st = torch.cuda.current_stream()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                out = fn(*args, **kw)
                e1.record(st)
                rec.append((name, e0, e1))
                return out
            return inner

        orig = tr.eng_v.backward, tr.eng_a.backward
        tr.eng_v.backward, tr.eng_a.backward = wrap(orig[0], "visual"), wrap(orig[1], "audio")
        per = []
        for _ in range(10):
            del rec[:]
            tr.step(*data[i % 4])
            i += 1
            torch.cuda.synchronize()
            t0 = min(rec, key=lambda r: rec[0][1].elapsed_time(r[1]))[1]
            per.append([(t0.elapsed_time(e0), t0.elapsed_time(e1)) for _, e0, e1 in rec])
            names = [n for n, _, _ in rec]
        tr.eng_v.backward, tr.eng_a.backward = orig
        chains[kind] = (names, np.median(np.array(per), axis=0))
    lines.append("# host time of one step() call on an idle device (enqueue only, no synchronise inside): "
                 + "; ".join(f"{k} {spread(v)} ms" for k, v in host.items()))
    lines.append(f"{'step':<16}{'ms median  (lowest .. highest)':<36}rounds")
    for kind, tr in trainers.items():
        try:  # (a run on random data may diverge: said in the table, the timing of such a run is of no use)
            r = tr.read()
            finite = bool(np.isfinite(r["loss_f"]))
        except FloatingPointError:
            r, finite = {}, False
        lines.append(f"{kind:<16}{spread(rounds[kind]):<36}" + " ".join(f"{x:.3f}" for x in rounds[kind]) + ("" if finite else "   NOT FINITE"))
        print(lines[-1], flush=True)
        if "pareto" in r:
            lines.append("#   last step's integration: " + "; ".join(
                f"{e}: branch {v['branch']}, gamma {v['gamma']:.4f}, s {v['s']:.4f}" for e, v in r["pareto"].items()))
    lines.append("# phases of a step on its main stream, ms (medians of 20 steps; device events): forwards (both chains joined) | junction "
                 "| head parameter gradients + backward chains (both joined; pareto: two backwards and the integration per chain) | "
                 "statistics, clip, update")
    for kind, v in phases.items():
        lines.append(f"#   {kind:<16}" + " | ".join(f"{x:.3f}" for x in v))
    lines.append("# the backward calls of a step on their own chains' streams, ms from the first one's begin (medians of 10 steps; in "
                 "the order the host enqueues them): begin .. end (duration)")
    for kind, (names, v) in chains.items():
        lines.append(f"#   {kind:<16}" + "; ".join(f"{n} {b:.3f} .. {e:.3f} ({e - b:.3f})" for n, (b, e) in zip(names, v)))
    m, p = rounds["mtl concat"], rounds["pareto concat"]
    lines.append(f"# pareto / mtl = {float(np.median(p)) / float(np.median(m)):.3f} (medians); added {float(np.median(p)) - float(np.median(m)):.3f} ms per step")
    sizes = {"audio": trainers["pareto concat"].pareto_range[0][1], "visual": trainers["pareto concat"].pareto_range[1][1]}
    for tr in trainers.values():
        tr.close()
    return sizes


def bench_integrate(a, dev, sizes, lines):
    lines.append(f"{'gdl_pareto_integrate, n':<40}{'us median  (lowest .. highest)':<36}{'GB/s at the median (20 n bytes)':<30}")
    lib = L.load()
    for e, n in sizes.items():
        gen = torch.Generator(device=dev).manual_seed(n % 1000)
        master = torch.randn(n + 8, generator=gen, device=dev)
        gms = [torch.empty_like(master) for _ in range(4)]
        gus = [0.5 * master + torch.randn(n + 8, generator=gen, device=dev) for _ in range(4)]
        info = torch.zeros(8, device=dev)
        nb = lib.gdl_pareto_workspace_bytes(n)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        st = L.cur_stream()

        def call(k):
            L.call("gdl_pareto_integrate", gms[k % 4].data_ptr() + 4, gus[k % 4].data_ptr() + 12, n, 0.5, L.ptr(info), L.ptr(ws), nb, st)

        us = []
        for _ in range(a.repeats):
            for gm in gms:
                gm.copy_(master)
            for k in range(8):
                call(k)
            for gm in gms:
                gm.copy_(master)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(a.launches):
                call(k)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) / a.launches * 1e3)
        med = float(np.median(us))
        lines.append(f"{e + ', ' + str(n):<40}{spread(us):<36}{20.0 * n / med / 1e3:<30.1f}")
        print(lines[-1], flush=True)


def bench_trees(a, lines):
    trees = {"this tree": ROOT, "parent": os.path.abspath(a.parent)}
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--no-extra",
           "--no-comparator", "--no-f32", "--no-prof"]
    ms = {k: [] for k in trees}
    for _ in range(a.bench_rounds):
        for k, d in trees.items():
            c = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=900)
            if c.returncode != 0:
                raise SystemExit(f"bench_pareto: bench.py failed in {d}:\n{c.stderr[-2000:]}")
            ms[k].append(float(json.loads(c.stdout.strip().splitlines()[-1])["ms_per_step"]))
            print(k, ms[k][-1], flush=True)
    lines.append(f"{'bench.py --gpus 1':<20}{'ms_per_step median  (lowest .. highest)':<44}runs")
    for k, v in ms.items():
        lines.append(f"{k:<20}{spread(v):<44}" + " ".join(f"{x:.3f}" for x in v))
    t, p = ms["this tree"], ms["parent"]
    d = float(np.median(t)) - float(np.median(p))
    sp = max(max(t) - min(t), max(p) - min(p))
    lines.append(f"# this tree - parent = {d:+.3f} ms (medians); the larger of the two trees' own spreads (highest - lowest) is {sp:.3f} ms: "
                 + ("the step did not move beyond the job's spread" if abs(d) <= sp else "the difference exceeds the job's spread"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit: its bench.py step beside this tree's")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pareto: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    lines = [f"# tools/bench_pareto.py on {torch.cuda.get_device_name(dev)}: CREMA-D shapes, B = {a.batch}, bf16, concat head, alpha 2.5, "
             f"{a.rounds} rounds x ({a.warmup} warm-up + {a.steps} timed steps) per trainer, the two alternating; ms per step"]
    sizes = bench_steps(a, dev, lines)
    torch.cuda.empty_cache()
    lines += ["#", f"# the integration alone: {a.repeats} repeats x {a.launches} back-to-back calls (two launches each), device events"]
    bench_integrate(a, dev, sizes, lines)
    torch.cuda.empty_cache()
    if a.parent:
        lines += ["#", f"# the benchmark step, pareto off: bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup} --no-extra "
                       f"--no-comparator --no-f32 --no-prof, fresh processes, this tree and the parent commit alternating, {a.bench_rounds} each"]
        bench_trees(a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
