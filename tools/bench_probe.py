#!/usr/bin/env python3
"""The linear probe (gdl.probe, csrc/linprobe.hip) on one MI355X: extraction throughput and the fused fit against the same
step composed in Python from the entry points the library had before it.

    python tools/bench_probe.py [--rounds 5] [--parent-tree DIR] [--out profiles/probe_bench.txt]
    python tools/bench_probe.py --spread          # CPU only: the float32 noise the kernel tests' bounds come from

1. gdl.extract_features: the eval-mode forward at B = 64, CREMA-D shapes (spec 257 x 188; 3 frames of 224 x 224), bf16, over
   `--batches` resident synthetic batches; samples per second of the whole call (the engine's planning included), host clock
   around a call that ends in a device synchronisation; median of the rounds with lowest and highest.
2. The fit at B = 64 and three sizes -- (N 6 698, n 6: CREMA-D's training split), (N 19 008, n 34: Kinetics-Sounds-sized),
   (N 20 000, n 309: a VGGSound-sized subset) -- on synthetic banks; ms per epoch and us per step:
     fused     gdl_linprobe_epoch, one C call per epoch (three launches per step);
     composed  per step: two torch gathers (features, labels), gdl_head_cls_ce, gdl_head_cls_bwd (df = NULL),
               gdl_optim_grad_stats, gdl_optim_sgd_step and one torch add for the epoch's loss -- built here only.
   Both are timed by the host clock around whole epochs ending in a device synchronisation, alternating per round; both end in
   the same state up to float32 summation order (checked: the largest deviation of W is printed).
3. With --parent-tree (a checkout of the parent commit, built): `bench.py --gpus 1` (the flagship step, which the probe is not
   part of) there and here, alternating, a fresh process each -- run BEFORE this process touches the device.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-gdl_amd"), os.path.join(ROOT, "tests")]

SIZES = ((6698, 6), (19008, 34), (20000, 309))
B = 64
HYPER = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4, max_norm=40.0)


def spread():
    """tests/probe_ref.py's cases: torch CPU float32 against the float64 restatement (docs/parity_log.md "Linear probe")"""
    import probe_ref as R
    import torch

    torch.set_num_threads(1)
    worst = {}
    for case in R.CASES:
        bank, labels, W, b, order = R.synthetic_case(*case)
        for mn in (40.0, R.CLIP_NORM):
            t64 = R.fit(bank, labels, order, W, b, max_norm=mn, **R.HYPER)
            t32 = R.torch_fit(bank, labels, order, W, b, max_norm=mn, **R.HYPER)
            d = {k: R.deviation(t32[-1][k], t64[-1][k]) for k in ("W", "b", "mW", "mb")}
            d["loss"] = max(R.loss_deviation(a["loss"], c["loss"]) for a, c in zip(t32, t64))
            norms = [x for t in t64 for x in t["norms"]]
            print(f"{str(case):16s} max_norm {mn:<5g} norms {min(norms):.3g} .. {max(norms):.3g}  " +
                  "  ".join(f"{k} {v:.2e}" for k, v in d.items()))
            for k, v in d.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("largest:  " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    print("bound 4x: " + "  ".join(f"{k} {4 * v:.3g}" for k, v in worst.items()))
    import numpy as np

    worst = {}
    for name in ("probe_audio_tiny", "probe_visual_tiny"):  # the fixtures' own torch float32 trajectories
        g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False)
        cfg = json.loads(str(g["config"]))
        for run, mn in (("n40", cfg["max_norm"]), ("clip", cfg["clip_norm"])):
            t64 = R.fit(g["features"], g["labels"], g["order"], g["W0"], g["b0"], lr=cfg["lr"], mu=cfg["momentum"],
                        wd=cfg["weight_decay"], max_norm=mn)
            for e, t in enumerate(t64):
                d = {k: R.deviation(g[f"{run}.e{e}.{k}"], t[k]) for k in ("W", "b", "mW", "mb")}
                d["loss"] = R.loss_deviation(g[f"{run}.e{e}.loss"], t["loss"])
                print(f"{name:18s} {run:4s} epoch {e}  " + "  ".join(f"{k} {v:.2e}" for k, v in d.items()))
                for k, v in d.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print("fixtures, largest: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def bench_py(tree, a):
    """ms per step of `bench.py --gpus 1` in `tree`, in a process of its own; a failure ends the whole run"""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup), "--no-extra",
           "--no-comparator", "--no-f32"]
    env = {k: v for k, v in os.environ.items() if k != "GDL_LIB"}
    p = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"bench_probe: bench.py in {tree} ended with {p.returncode}:\n{p.stderr[-2000:]}")
    return float(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])


def bench_parent(a, lines):
    here, parent = [], []
    for k in range(a.pairs):  # (the order within a pair alternates)
        for tree in ((a.parent_tree, ROOT) if k % 2 == 0 else (ROOT, a.parent_tree)):
            (here if tree == ROOT else parent).append(bench_py(tree, a))
        print(f"bench.py: parent {parent[-1]:.3f} ms, this tree {here[-1]:.3f} ms", flush=True)
    sp = max(max(parent) - min(parent), max(here) - min(here))
    d = sum(here) / len(here) - sum(parent) / len(parent)
    lines += ["parent commit     " + " ".join(f"{x:8.3f}" for x in parent), "this commit       " + " ".join(f"{x:8.3f}" for x in here),
              f"# this - parent (means) = {d:+.4f} ms; spread between the runs of one tree = {sp:.4f} ms: the default step "
              f"{'DIFFERS BY MORE THAN' if abs(d) > sp else 'lies within'} the job's own spread"]


def med(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def bench_extract(a, dev, lines):
    import argparse as ap

    import gdl
    import torch
    from models.basic_model import AVClassifier_DGL

    torch.manual_seed(0)
    model = AVClassifier_DGL(ap.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=B)).to(dev)
    distinct = 4
    specs = [torch.randn(B, 257, 188, device=dev) for _ in range(distinct)]
    images = [torch.randn(B, 3, 3, 224, 224, device=dev) for _ in range(distinct)]
    labels = [torch.randint(0, 6, (B,), device=dev) for _ in range(distinct)]
    lines += ["extract_features        samples/s median     low    high   ms per batch of 64"]
    for modality in ("audio", "visual"):
        batches = [(specs[i % distinct], images[i % distinct], labels[i % distinct]) for i in range(a.batches)]
        rates = []
        for r in range(a.rounds + 1):  # (round 0: warm-up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bank = gdl.extract_features(model, modality, batches, dtype="bf16")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r:
                rates.append(bank.N / dt)
        lines += [f"{modality:22s} {med(rates):16.0f} {min(rates):7.0f} {max(rates):7.0f}   {1e3 * B / med(rates):.3f}"]
        print(lines[-1], flush=True)


class Composed:
    """The probe's step from the entry points the library had without gdl_linprobe_epoch"""

    def __init__(self, bank, labels, W, b, dev):
        import torch
        from gdl import _lib as L

        self.L, self.lib, self.torch = L, L.load(), torch
        n = W.shape[0]
        self.n, self.bank, self.labels = n, bank, labels
        tot = n * 512 + n
        self.p, self.g, self.m = torch.empty(tot, device=dev), torch.empty(tot, device=dev), torch.zeros(tot, device=dev)
        self.p[:n * 512].copy_(W.reshape(-1))
        self.p[n * 512:].copy_(b)
        offs = (ctypes.c_int64 * 3)(0, n * 512, tot)
        grp = (ctypes.c_int32 * 2)(0, 0)
        self.h = ctypes.c_void_p()
        L.call("gdl_optim_create", ctypes.byref(self.h), offs, grp, 2)
        self.wsb = self.lib.gdl_optim_workspace_bytes(self.h)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        self.stats = torch.zeros(self.lib.gdl_optim_stats_len(self.h), device=dev)
        self.f, self.y = torch.empty((B, 512), device=dev), torch.empty(B, dtype=torch.int64, device=dev)
        self.out, self.dl, self.df = torch.empty((B, n), device=dev), torch.empty((B, n), device=dev), torch.empty((B, 512), device=dev)
        self.loss, self.acc = torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)

    def epoch(self, order64, lr, momentum, weight_decay, max_norm):
        """order64: [steps, B] int64 on the device"""
        L, torch, n = self.L, self.torch, self.n
        st = L.cur_stream()
        p, g = self.p.data_ptr(), self.g.data_ptr()
        for s in range(order64.shape[0]):
            torch.index_select(self.bank, 0, order64[s], out=self.f)
            torch.index_select(self.labels, 0, order64[s], out=self.y)
            L.call("gdl_head_cls_ce", L.ptr(self.f), p, p + 4 * n * 512, L.ptr(self.y), 1.0, L.ptr(self.out), L.ptr(self.loss),
                   L.ptr(self.dl), L.ptr(self.df), B, n, 512, st)
            L.call("gdl_head_cls_bwd", L.ptr(self.f), p, L.ptr(self.dl), None, g, g + 4 * n * 512, B, n, 512, st)
            L.call("gdl_optim_grad_stats", self.h, g, max_norm, 1.0, L.ptr(self.stats), L.ptr(self.ws), self.wsb, st)
            L.call("gdl_optim_sgd_step", self.h, p, g, L.ptr(self.m), L.ptr(self.stats), 1.0, lr, momentum, weight_decay, st)
            self.acc += self.loss


def bench_fit(a, dev, lines):
    import gdl
    import numpy as np
    import torch

    lines += ["fit, B = 64            steps   fused ms/epoch median (low high)   us/step | composed ms/epoch median (low high)   us/step"
              " | composed / fused | max dev W"]
    for N, n in SIZES:
        g = torch.Generator().manual_seed(N)
        bank = gdl.FeatureBank(torch.randn((N, 512), generator=g).abs().to(dev), torch.randint(0, n, (N,), generator=g).to(dev))
        probe = gdl.LinearProbe(n, dev, seed=0)
        comp = Composed(bank.features, bank.labels, probe.weight, probe.bias, dev)
        steps = N // B
        tf, tc = [], []
        for r in range(a.rounds + 1):  # (round 0: warm-up; both fits see the same tables)
            tab = gdl.probe_order(N, B, a.epochs, torch.Generator().manual_seed(r))
            tab64 = tab.to(dev).long()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            probe.fit(bank, a.epochs, batch_size=B, order=tab, **HYPER)  # (ends in its one synchronisation)
            t1 = time.perf_counter()
            for e in range(a.epochs):
                comp.epoch(tab64[e], HYPER["lr"], HYPER["momentum"], HYPER["weight_decay"], HYPER["max_norm"])
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r:
                tf.append(1e3 * (t1 - t0) / a.epochs)
                tc.append(1e3 * (t2 - t1) / a.epochs)
        Wc = comp.p[:n * 512].view(n, 512).cpu().numpy().astype(np.float64)
        Wf = probe.weight.cpu().numpy().astype(np.float64)
        dev_w = float(np.abs(Wc - Wf).max() / np.abs(Wf).max())
        lines += [f"N {N:6d} n {n:3d}      {steps:6d}   {med(tf):9.3f} ({min(tf):.3f} {max(tf):.3f})   {1e3 * med(tf) / steps:7.2f} | "
                  f"{med(tc):9.3f} ({min(tc):.3f} {max(tc):.3f})   {1e3 * med(tc) / steps:7.2f} | {med(tc) / med(tf):6.2f}x | {dev_w:.2e}"]
        print(lines[-1], flush=True)
        comp.lib.gdl_optim_destroy(comp.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spread", action="store_true", help="CPU only: print the float32-vs-float64 deviations of the test cases")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=3, help="timed epochs per round and fit")
    ap.add_argument("--batches", type=int, default=16, help="batches of 64 per extract_features call")
    ap.add_argument("--steps", type=int, default=100, help="bench.py --steps (section 3)")
    ap.add_argument("--warmup", type=int, default=20, help="bench.py --warmup (section 3)")
    ap.add_argument("--pairs", type=int, default=3, help="bench.py runs per tree (section 3)")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.spread:
        return spread()
    parent_lines = []
    if a.parent_tree:
        bench_parent(a, parent_lines)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_probe: no GPU visible; there is nothing to time on a CPU (--spread is the CPU mode)")
    dev = "cuda:0"
    lines = [f"# tools/bench_probe.py on {torch.cuda.get_device_name(0)}",
             f"# 1. gdl.extract_features, eval-mode forward, B = {B}, CREMA-D shapes, bf16, {a.batches} batches per call "
             f"({a.batches * B} samples); {a.rounds} rounds after one warm-up call; host clock around the call + one synchronisation"]
    bench_extract(a, dev, lines)
    lines += ["#", f"# 2. the fit: {a.rounds} rounds after one warm-up round, {a.epochs} epochs per round and fit, fused and composed "
              "alternating on the same order tables; host clock around whole epochs ending in a synchronisation.",
              "#    composed = per step 2 torch gathers + gdl_head_cls_ce + gdl_head_cls_bwd + gdl_optim_grad_stats + gdl_optim_sgd_step"
              " + 1 torch add; max dev W = max |W composed - W fused| / max |W| after all rounds"]
    bench_fit(a, dev, lines)
    if parent_lines:
        lines += ["#", f"# 3. bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup} --no-extra --no-comparator --no-f32 (the flagship step; the "
                  "probe is not part of it) on a checkout of the parent commit and on this commit, alternating in one job on the same "
                  "box, a process each, before section 1; ms per step"] + parent_lines
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
