#!/usr/bin/env python3
"""The unimodal baselines' step (audio only, visual only) beside the full DGL concat step, and the fused classifier launch
beside gdl_head_uni_dfeat, on one MI355X.

    python tools/bench_unimodal.py [--rounds 3] [--steps 100] [--warmup 20] [--out profiles/unimodal_bench.txt]

Steps: CREMA-D shapes (spec 257 x 188, 3 frames of 224 x 224), B = 64, bf16 encoders, seeded weight_init as main.py /
main_dgl.py build the model.  Three trainers live in the process -- UnimodalTrainer on AVClassifier_DGL(modality='audio'),
on modality='visual', and DGLTrainer on modality='full' (the step bench.py times) -- and are timed alternately: per round and
trainer `warmup` untimed and `steps` timed steps between two device synchronisations (host clock); the median over the rounds
is reported.  A unimodal step is a strict subset of the DGL step's work, so each must read below it.

Kernels: gdl_head_cls_ce (logits, loss, dlogits, df) against gdl_head_uni_dfeat (df alone; the same chain work minus three
small stores and the loss) at (B, n) = (64, 6) and (64, 309), alternated: per repeat `--launches` back-to-back launches on one
stream between two device events, microseconds per launch; min / median / max over `--repeats` repeats is the spread.
Back-to-back launches of a 64-block kernel overlap their tails, so this is the launch-to-launch rate, the same for both.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-gdl_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gdl.trainer import DGLTrainer  # noqa: E402
from gdl.unimodal import UnimodalTrainer  # noqa: E402


def build(modality, wl, batch, dev):
    from models.basic_model import AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    setup_seed(0)
    args = argparse.Namespace(fusion_method="concat", dataset=wl["dataset"], modality=modality, batch_size=batch)
    model = AVClassifier_DGL(args)
    model.apply(weight_init)
    return model.to(dev).train()


def bench_steps(a, dev, lines):
    wl, B = bench.WORKLOADS["cremad"], a.batch
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]
    trainers = {
        "audio-only": UnimodalTrainer(build("audio", wl, B, dev), lr=2e-3, dtype="bf16"),
        "visual-only": UnimodalTrainer(build("visual", wl, B, dev), lr=2e-3, dtype="bf16"),
        "dgl concat": DGLTrainer(build("full", wl, B, dev), lr=2e-3, alpha=wl["alpha"], max_norm=40.0, dtype="bf16"),
    }
    rounds = {k: [] for k in trainers}
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
    lines.append(f"{'step':<14}{'ms':>8}{'of dgl':>9}   rounds")
    ms = {k: float(np.median(v)) for k, v in rounds.items()}
    for kind, tr in trainers.items():
        try:  # (a run on random data may diverge: said in the table, the timing of such a run is of no use)
            finite = bool(np.isfinite(tr.read()["loss_f"]))
        except FloatingPointError:
            finite = False
        tr.close()
        lines.append(f"{kind:<14}{ms[kind]:>8.3f}{ms[kind] / ms['dgl concat']:>9.3f}   " + " ".join(f"{x:.3f}" for x in rounds[kind])
                     + ("" if finite else "   NOT FINITE"))
        print(lines[-1], flush=True)
    worst = {k: max(rounds[k]) for k in ("audio-only", "visual-only")}
    ok = all(v < min(rounds["dgl concat"]) for v in worst.values())
    lines.append("# every round of each unimodal step is shorter than every round of the DGL step: " + ("yes" if ok else "NO"))


def bench_kernels(a, dev, lines):
    B = a.batch
    lines.append(f"{'kernel, (B, n)':<34}{'us min':>8}{'median':>8}{'max':>8}")
    for n in (6, 309):
        gen = torch.Generator(device=dev).manual_seed(n)
        f = torch.randn(B, 512, generator=gen, device=dev).clamp_min(0)
        W = torch.randn(n, 512, generator=gen, device=dev) * 0.05
        b = torch.randn(n, generator=gen, device=dev) * 0.1
        lab = torch.randint(0, n, (B,), generator=gen, device=dev)
        out, dl, df = torch.empty(B, n, device=dev), torch.empty(B, n, device=dev), torch.empty(B, 512, device=dev)
        loss = torch.empty(1, device=dev)
        st = L.cur_stream()
        calls = {
            "gdl_head_cls_ce": lambda: L.call("gdl_head_cls_ce", L.ptr(f), L.ptr(W), L.ptr(b), L.ptr(lab), 1.0, L.ptr(out),
                                              L.ptr(loss), L.ptr(dl), L.ptr(df), B, n, 512, st),
            "gdl_head_uni_dfeat": lambda: L.call("gdl_head_uni_dfeat", L.ptr(f), L.ptr(W), 512, L.ptr(b), L.ptr(lab), 1.0,
                                                 L.ptr(df), B, n, st),
        }
        us = {k: [] for k in calls}
        for _ in range(a.repeats):
            for k, fn in calls.items():
                for _ in range(50):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                e1.synchronize()
                us[k].append(e0.elapsed_time(e1) / a.launches * 1e3)
        for k, v in us.items():
            lines.append(f"{k + ', (' + str(B) + ', ' + str(n) + ')':<34}{min(v):>8.2f}{float(np.median(v)):>8.2f}{max(v):>8.2f}")
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unimodal: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    lines = [f"# tools/bench_unimodal.py on {torch.cuda.get_device_name(dev)}: CREMA-D shapes, B = {a.batch}, bf16, "
             f"{a.rounds} rounds x ({a.warmup} warm-up + {a.steps} timed steps) per trainer, the three alternating;",
             "# ms per step = median over the rounds"]
    bench_steps(a, dev, lines)
    torch.cuda.empty_cache()
    lines += ["#", f"# the fused classifier launch beside the DGL step's gdl_head_uni_dfeat, {a.repeats} repeats x {a.launches} "
              "back-to-back launches, alternating; us per launch (device events)"]
    bench_kernels(a, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
