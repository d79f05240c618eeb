#!/usr/bin/env python3
"""Prototypical modal rebalance (csrc/proto.hip) alone and inside the B = 64 CREMA-D joint step, on one MI355X.

    python tools/bench_pmr.py [--rounds 5] [--steps 100] [--warmup 20] [--parent-tree DIR] [--out profiles/pmr_bench.txt]

1. The three launches alone, back-to-back between two device events, us per launch: gdl_proto_ce (one modality) and
   gdl_proto_apply at B = 64 with n = 6 (CREMA-D), 34 (Kinetics-Sounds) and 309 (VGGSound) classes; gdl_proto_update on banks of
   N = 2 560 and 15 360 rows (uniform random labels) at the same class counts.
2. The joint step (concat head, bf16, spec 257 x 188, 3 frames of 224 x 224, synthetic batches) of ONE trainer with prototypes
   attached, timed against itself: windows with the epoch outside the modulation window (the step is then the plain joint step,
   launch for launch) and inside it, alternating, the order swapped from round to round.  Same trainer, same memory, same
   streams: the difference is what the two gdl_proto_ce and the one gdl_proto_apply cost the step; the spread between rounds of
   one setting is the noise floor.  Per round and setting `warmup` untimed and `steps` timed steps, host clock around the steps
   and one device synchronisation.
3. With --parent-tree (a checkout of the parent commit, built): `bench.py --gpus 1` (the flagship DGL step; it never passes
   `prototypes`) there and here, alternating, a fresh process each -- run BEFORE this process touches the device.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-gdl_amd")]


def bench_py(tree, a):
    """ms per step of `bench.py --gpus 1` in `tree`, in a process of its own; a failure ends the whole run"""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup), "--no-extra",
           "--no-comparator", "--no-f32"]
    env = {k: v for k, v in os.environ.items() if k != "GDL_LIB"}
    p = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"bench_pmr: bench.py in {tree} ended with {p.returncode}:\n{p.stderr[-2000:]}")
    return float(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])


def bench_parent(a, lines):
    here, parent = [], []
    for k in range(a.pairs):  # (the order within a pair alternates: neither tree always runs on the warmer device)
        for tree in ((a.parent_tree, ROOT) if k % 2 == 0 else (ROOT, a.parent_tree)):
            (here if tree == ROOT else parent).append(bench_py(tree, a))
        print(f"bench.py: parent {parent[-1]:.3f} ms, this tree {here[-1]:.3f} ms", flush=True)
    sp = max(max(parent) - min(parent), max(here) - min(here))
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else sum(sorted(v)[len(v) // 2 - 1:len(v) // 2 + 1]) / 2  # noqa: E731
    d = med(here) - med(parent)
    lines += ["parent commit     " + " ".join(f"{x:8.3f}" for x in parent) + f"   median {med(parent):.3f}",
              "this commit       " + " ".join(f"{x:8.3f}" for x in here) + f"   median {med(here):.3f}",
              f"# this - parent (medians) = {d:+.4f} ms; spread between the runs of one tree = {sp:.4f} ms: the default step "
              f"{'DIFFERS BY MORE THAN' if abs(d) > sp else 'lies within'} the job's own spread"]


def timed(fn, a):
    """us per launch of fn: (min, median, max) over a.repeats windows of a.launches back-to-back launches"""
    import numpy as np
    import torch

    us = []
    for _ in range(a.repeats):
        for _ in range(50):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) / a.launches * 1e3)
    return min(us), float(np.median(us)), max(us)


def bench_kernels(a, dev, lines):
    import torch

    from gdl import _lib as L

    st = L.cur_stream()
    B = a.batch
    g = torch.Generator(device="cpu").manual_seed(7)
    f = (0.5 * torch.randn(B, 512, generator=g).abs()).to(dev)
    lines.append(f"{'launch alone':<36}{'us min':>9}{'median':>9}{'max':>9}")
    for n in (6, 34, 309):
        P = (0.5 * torch.randn(n, 512, generator=g).abs()).to(dev)
        lab = torch.randint(0, n, (B,), generator=g).to(dev)
        u, terms, stats = torch.empty((2, B, 512), device=dev), torch.empty((2, 2, B), device=dev), torch.empty(8, device=dev)
        dfa, dfv = torch.zeros((B, 512), device=dev), torch.zeros((B, 512), device=dev)

        def ce(m=0):
            L.call("gdl_proto_ce", f.data_ptr(), P.data_ptr(), lab.data_ptr(), u[m].data_ptr(), terms[m].data_ptr(), None, B, n, 512, st)

        ce(1)

        def apply():
            L.call("gdl_proto_apply", terms[0].data_ptr(), terms[1].data_ptr(), u[0].data_ptr(), u[1].data_ptr(), dfa.data_ptr(),
                   dfv.data_ptr(), 1e-3, stats.data_ptr(), B, 512, st)

        terms[1, 0] *= 0.5  # (audio ahead: one side is applied, as in a step)
        for name, fn in ((f"gdl_proto_ce     B={B} n={n}", ce), (f"gdl_proto_apply  B={B} n={n}", apply)):
            lo, med, hi = timed(fn, a)
            lines.append(f"{name:<36}{lo:>9.2f}{med:>9.2f}{hi:>9.2f}")
            print(lines[-1], flush=True)
    for N in (2560, 15360):
        bank = (0.5 * torch.randn(N, 512, generator=g).abs()).to(dev)
        for n in (6, 34, 309):
            lab = torch.randint(0, n, (N,), generator=g).to(dev)
            P = torch.zeros((n, 512), device=dev)
            cnt, info = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)

            def update():
                L.call("gdl_proto_update", bank.data_ptr(), lab.data_ptr(), N, P.data_ptr(), n, 512, 0.2, 0, cnt.data_ptr(),
                       info.data_ptr(), st)

            lo, med, hi = timed(update, argparse.Namespace(repeats=a.repeats, launches=max(a.launches // 10, 10)))
            lines.append(f"{f'gdl_proto_update N={N} n={n}':<36}{lo:>9.2f}{med:>9.2f}{hi:>9.2f}")
            print(lines[-1], flush=True)


def bench_step(a, dev, lines):
    import numpy as np
    import torch

    import bench
    import gdl
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier
    from utils.utils import setup_seed, weight_init

    wl, B = bench.WORKLOADS["cremad"], a.batch
    n = wl["n_classes"]
    setup_seed(0)
    model = AVClassifier(argparse.Namespace(fusion_method="concat", dataset=wl["dataset"], modality="full", batch_size=B))
    model.apply(weight_init)
    model = model.to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, n, (B,), generator=g).to(dev)) for _ in range(4)]
    protos = gdl.Prototypes(n, dev)
    protos.protos.copy_(0.5 * torch.randn(2, n, 512, generator=g).abs())
    protos.updates = 1
    tr = DGLTrainer(model, lr=2e-3, max_norm=40.0, dtype="bf16", mode="joint", prototypes=protos, alpha=1.0, modulation_starts=0,
                    modulation_ends=0)
    t = {False: [], True: []}
    i = 0
    for r in range(a.rounds):
        for on in ((False, True) if r % 2 == 0 else (True, False)):
            tr.epoch = 0 if on else 1
            for _ in range(a.warmup):
                tr.step(*data[i % 4])
                i += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step(*data[i % 4])
                i += 1
            torch.cuda.synchronize()
            t[on].append((time.perf_counter() - t0) / a.steps * 1e3)
            assert ("pmr" in tr.read()) == on
    tr.close()
    off, on = float(np.median(t[False])), float(np.median(t[True]))
    floor = max(max(t[False]) - min(t[False]), max(t[True]) - min(t[True]))
    lines += [f"{'joint step, one trainer':<26}{'ms median':>10}{'min':>8}{'max':>8}   rounds",
              f"{'outside the window':<26}{off:>10.3f}{min(t[False]):>8.3f}{max(t[False]):>8.3f}   " + " ".join(f"{x:.3f}" for x in t[False]),
              f"{'inside (PMR on)':<26}{on:>10.3f}{min(t[True]):>8.3f}{max(t[True]):>8.3f}   " + " ".join(f"{x:.3f}" for x in t[True]),
              f"# on - off (medians) = {on - off:+.4f} ms ({(on - off) / off * 100:+.2f} %); spread between rounds of one setting = "
              f"{floor:.4f} ms: the difference {'EXCEEDS' if on - off > floor else 'is within'} it"]
    print("\n".join(lines[-4:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: bench.py there and here (section 3)")
    ap.add_argument("--pairs", type=int, default=4, help="bench.py runs per tree in section 3")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    parent_lines = []
    if a.parent_tree:  # fresh processes, before this one opens the device
        bench_parent(a, parent_lines)
    import torch

    from gdl import _lib as L

    if not torch.cuda.is_available():
        raise SystemExit("bench_pmr: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    lines = [f"# tools/bench_pmr.py on {torch.cuda.get_device_name(dev)}",
             f"# 1. the three launches alone: {a.repeats} repeats x {a.launches} back-to-back launches ({max(a.launches // 10, 10)} for "
             "gdl_proto_update), us per launch (device events); gdl_proto_ce is ONE modality's launch, a step has two on two streams"]
    bench_kernels(a, dev, lines)
    lines += ["#", f"# 2. the joint step, CREMA-D shapes, B = {a.batch}, bf16, concat head, ONE trainer with prototypes attached: {a.rounds} "
              f"rounds x ({a.warmup} warm-up + {a.steps} timed steps) per setting, alternating, the order swapped every round; ms per step"]
    bench_step(a, dev, lines)
    if parent_lines:
        lines += ["#", f"# 3. bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup} --no-extra --no-comparator --no-f32 (the flagship DGL "
                  "step; no prototypes there) on a checkout of the parent commit and on this commit, alternating in one job on the same "
                  "box, a process each, before section 1; ms per step"] + parent_lines
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
