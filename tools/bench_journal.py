#!/usr/bin/env python3
"""The step journal (csrc/journal.hip) alone and inside the B = 64 CREMA-D DGL step, on one MI355X.

    python tools/bench_journal.py [--rounds 5] [--steps 100] [--warmup 20] [--parent-tree DIR] [--out profiles/journal_bench.txt]

1. gdl_journal_append alone at the sizes a step launches it with -- n_logits = 384 (64 x 6, CREMA-D), 1 984 (64 x 31,
   Kinetics-Sounds), 19 776 (64 x 309, VGGSound) -- back-to-back launches between two device events, us per launch.
2. The DGL step (concat head, bf16, spec 257 x 188, 3 frames of 224 x 224, synthetic batches), FOUR trainers in one process, two
   of each kind, timed alternately (per round and trainer `warmup` untimed and `steps` timed steps, host clock; median over the
   rounds):
     (a) journal off, no reads: the steps, then one device synchronisation;
     (b) journal on, no reads: the steps, then `tr.journal()` -- its one synchronisation and one host copy are inside the time;
     (c) journal off, `read()` after every step: what the script's per-step log costs on the runner today (timed on the two
         (a) trainers, in windows of their own).
   The difference between the two trainers of ONE kind is the run's own spread, the yardstick profiles/ablation_bench.txt uses;
   (b) - (a) is read against it, (c) - (a) is what the journal saves.
   2b. Where a trainer was built in the process has moved its step by up to 0.9 ms in such four-trainer runs
   (profiles/diversity_bench.txt), far more than one small launch can cost.  So each (b) trainer is also timed against ITSELF:
   windows with its journal detached (`tr._journal = None`: the step then takes the journal=0 path, launch for launch) and
   attached, alternating, the order swapped from round to round.  Same trainer, same memory, same streams: the difference
   is the launch's, the spread between rounds of one setting the noise floor.
3. With --parent-tree (a checkout of the parent commit, built): `bench.py --gpus 1` (the flagship step; it never passes the
   switch) there and here, alternating, a fresh process each -- run BEFORE this process touches the device.
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
        raise SystemExit(f"bench_journal: bench.py in {tree} ended with {p.returncode}:\n{p.stderr[-2000:]}")
    return float(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])


def bench_parent(a, lines):
    here, parent = [], []
    for k in range(a.pairs):  # (the order within a pair alternates: neither tree always runs on the warmer device)
        for tree in ((a.parent_tree, ROOT) if k % 2 == 0 else (ROOT, a.parent_tree)):
            (here if tree == ROOT else parent).append(bench_py(tree, a))
        print(f"bench.py: parent {parent[-1]:.3f} ms, this tree {here[-1]:.3f} ms", flush=True)
    sp = max(max(parent) - min(parent), max(here) - min(here))
    d = sum(here) / len(here) - sum(parent) / len(parent)
    lines += [f"parent commit     " + " ".join(f"{x:8.3f}" for x in parent), f"this commit       " + " ".join(f"{x:8.3f}" for x in here),
              f"# this - parent (means) = {d:+.4f} ms; spread between the runs of one tree = {sp:.4f} ms: the default step "
              f"{'DIFFERS BY MORE THAN' if abs(d) > sp else 'lies within'} the job's own spread"]


def build(wl, batch, dev):
    """The model as main_dgl.py:230-246 builds it (seeded weight_init)."""
    from models.basic_model import AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    setup_seed(0)
    model = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset=wl["dataset"], modality="full", batch_size=batch))
    model.apply(weight_init)
    return model.to(dev).train()


def bench_kernel(a, dev, lines):
    import numpy as np
    import torch

    from gdl import _lib as L

    lines.append(f"{'kernel alone: n_logits':<28}{'us min':>8}{'median':>8}{'max':>8}")
    st = L.cur_stream()
    cap = 128
    buf = torch.zeros(L.load().gdl_journal_bytes(cap), dtype=torch.uint8, device=dev)
    src = torch.rand(16, device=dev)
    for n in (384, 1984, 19776):
        oa, ov = torch.randn(n, device=dev), torch.randn(n, device=dev)

        def fn():
            L.call("gdl_journal_append", buf.data_ptr(), cap, src.data_ptr(), 3, src.data_ptr() + 12, oa.data_ptr(), ov.data_ptr(), n,
                   src.data_ptr() + 28, src.data_ptr() + 32, src.data_ptr() + 36, st)

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
        lines.append(f"{n:<28}{min(us):>8.2f}{float(np.median(us)):>8.2f}{max(us):>8.2f}")
        print(lines[-1], flush=True)


def bench_steps(a, dev, lines):
    import numpy as np
    import torch

    import bench
    from gdl.trainer import DGLTrainer

    wl, B = bench.WORKLOADS["cremad"], a.batch
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]
    kw = dict(lr=2e-3, max_norm=40.0, dtype="bf16", alpha=wl["alpha"])
    trainers = {f"({'b' if on else 'a'}) journal {'on' if on else 'off'} {tag}": DGLTrainer(build(wl, B, dev), journal=on, **kw)
                for tag in ("A", "B") for on in (0, a.warmup + a.steps)}
    rounds = {k: [] for k in trainers}
    rounds.update({k.replace("(a) journal off", "(c) off + read()"): [] for k in trainers if k.startswith("(a)")})
    i = 0
    last = {}
    for _ in range(a.rounds):
        for kind, tr in trainers.items():
            on = kind.startswith("(b)")
            for every in ((False, True) if not on else (False,)):
                for _ in range(a.warmup):
                    tr.step(*data[i % 4])
                    i += 1
                torch.cuda.synchronize()
                if on:
                    tr.journal()  # a new epoch: the timed window is one epoch of `steps` rows
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    tr.step(*data[i % 4])
                    i += 1
                    if every:
                        tr.read()
                if on:
                    last[kind] = tr.journal()
                else:
                    torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / a.steps * 1e3
                rounds[kind.replace("(a) journal off", "(c) off + read()") if every else kind].append(dt)
    ms = {k: float(np.median(v)) for k, v in rounds.items()}
    lines.append(f"{'DGL step':<26}{'ms':>8}   rounds")
    for kind in sorted(rounds):
        extra = ""
        if kind in last:
            j = last[kind]
            extra = (f"   last epoch: count {j['count']}, dropped {j['dropped']}, mean loss_f {j['means']['loss_f']:.4f}, "
                     f"mean |out_a| {j['means']['abs_out_a']:.4f}")
            assert j["count"] == a.steps and j["dropped"] == 0 and np.isfinite(j["rows"][:, :9]).all()
        lines.append(f"{kind:<26}{ms[kind]:>8.3f}   " + " ".join(f"{x:.3f}" for x in rounds[kind]) + extra)
        print(lines[-1], flush=True)
    self_ms = {}
    for kind, tr in trainers.items():
        if not kind.startswith("(b)"):
            continue
        jn, t = tr._journal, {False: [], True: []}
        for r in range(a.rounds):
            for attached in ((False, True) if r % 2 == 0 else (True, False)):
                tr._journal = jn if attached else None
                for _ in range(a.warmup):
                    tr.step(*data[i % 4])
                    i += 1
                torch.cuda.synchronize()
                if attached:
                    tr.journal()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    tr.step(*data[i % 4])
                    i += 1
                if attached:
                    assert tr.journal()["count"] == a.steps
                else:
                    torch.cuda.synchronize()
                t[attached].append((time.perf_counter() - t0) / a.steps * 1e3)
        tr._journal = jn
        self_ms[kind] = t
    for tr in trainers.values():
        tr.close()
    A = [ms[k] for k in sorted(ms) if k.startswith("(a)")]
    Bm = [ms[k] for k in sorted(ms) if k.startswith("(b)")]
    C = [ms[k] for k in sorted(ms) if k.startswith("(c)")]
    a_, b_, c_ = sum(A) / 2, sum(Bm) / 2, sum(C) / 2
    spread = max(abs(A[0] - A[1]), abs(Bm[0] - Bm[1]))
    lines += [f"# (b) - (a) = {b_ - a_:+.4f} ms ({(b_ - a_) / a_ * 100:+.2f} %), pair by pair {Bm[0] - A[0]:+.4f} (A) {Bm[1] - A[1]:+.4f} (B); "
              f"noise floor = spread between two trainers of one kind = {spread:.4f} ms: the journal's cost "
              f"{'EXCEEDS' if b_ - a_ > spread else 'is within'} the run's own spread",
              f"# (c) - (a) = {c_ - a_:+.4f} ms ({(c_ - a_) / a_ * 100:+.2f} %), pair by pair {C[0] - A[0]:+.4f} (A) {C[1] - A[1]:+.4f} (B): "
              "what read() after every step costs, and the journal saves",
              "#", "# 2b. each (b) trainer against itself: journal detached / attached in alternating windows; ms per step, median over the rounds",
              f"{'same trainer':<26}{'detached':>9}{'attached':>9}{'diff':>9}   rounds detached | attached"]
    for kind, t in self_ms.items():
        d, o = float(np.median(t[False])), float(np.median(t[True]))
        floor = max(max(t[False]) - min(t[False]), max(t[True]) - min(t[True]))
        lines.append(f"{kind:<26}{d:>9.3f}{o:>9.3f}{o - d:>+9.4f}   " + " ".join(f"{x:.3f}" for x in t[False]) + " | " +
                     " ".join(f"{x:.3f}" for x in t[True]) + f"   (spread between rounds of one setting {floor:.4f} ms: the difference "
                     f"{'EXCEEDS' if o - d > floor else 'is within'} it)")
        print(lines[-1], flush=True)


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
        raise SystemExit("bench_journal: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    lines = [f"# tools/bench_journal.py on {torch.cuda.get_device_name(dev)}",
             f"# 1. gdl_journal_append alone (one 256-thread block; both logit sets, every source present): {a.repeats} repeats x "
             f"{a.launches} back-to-back launches, us per launch (device events)"]
    bench_kernel(a, dev, lines)
    lines += ["#", f"# 2. the DGL step, CREMA-D shapes, B = {a.batch}, bf16, concat head: {a.rounds} rounds x ({a.warmup} warm-up + "
              f"{a.steps} timed steps) per trainer and window, the four trainers alternating; ms per step = median over the rounds.",
              "#    (a) journal=0, no reads, one device synchronisation at the end of the window (this commit with the switch off; NOT "
              "a timing of the parent commit: that is section 3);",
              f"#    (b) journal={a.warmup + a.steps}, no reads, tr.journal() at the end of the window, inside the time (one synchronisation, one "
              "host copy);",
              "#    (c) the (a) trainers with read() after every step (a synchronisation and five or more host copies per step)"]
    bench_steps(a, dev, lines)
    if parent_lines:
        lines += ["#", f"# 3. bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup} --no-extra --no-comparator --no-f32 (the flagship step; "
                  "the switch is off there) on a checkout of the parent commit and on this commit, alternating in one job on the same "
                  "box, a process each, before section 1; ms per step"] + parent_lines
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
