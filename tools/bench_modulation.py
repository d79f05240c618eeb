#!/usr/bin/env python3
"""Joint-training step with and without OGM / OGM-GE gradient modulation on one MI355X.

    python tools/bench_modulation.py [--rounds 5] [--steps 100] [--warmup 20] [--out profiles/modulation_bench.txt]

CREMA-D shapes (spec 257 x 188, 3 frames of 224 x 224), B = 64, bf16 encoders, concat head.  Three trainers live in the process:
DGLTrainer(AVClassifier(args), mode="joint", modulation=m, alpha=0.8) for m in Normal, OGM, OGM_GE.  They are timed alternately:
per round and trainer `warmup` untimed and `steps` timed steps between two device synchronisations (host clock); the median
over the rounds is reported.  "Normal" issues exactly the launches of a trainer built without the modulation arguments, so it is
the yardstick the other two are read against.  All three run without the visual engine's own weight-gradient side stream (as
tools/bench_joint_heads.py: one stream layout for every trainer of the process).  What the modulation adds per step: one
launch for the unimodal scores behind the head forward, and between the gradient statistics and the update one read of the
marked gradients (OGM_GE: their sum), one block for the coefficients and sigmas, one read + write of the arena.
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
from gdl.trainer import MODULATIONS, DGLTrainer  # noqa: E402


def build(wl, batch, dev):
    from models.basic_model import AVClassifier
    from utils.utils import setup_seed, weight_init

    setup_seed(0)
    args = argparse.Namespace(fusion_method="concat", dataset=wl["dataset"], modality="full", batch_size=batch)
    model = AVClassifier(args)
    model.apply(weight_init)
    return model.to(dev).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_modulation: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    wl, B = bench.WORKLOADS["cremad"], a.batch
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]
    trainers = {m: DGLTrainer(build(wl, B, dev), lr=2e-3, alpha=0.8, max_norm=40.0, dtype="bf16", mode="joint",
                              visual_side_stream=False, modulation=m) for m in MODULATIONS}
    rounds = {m: [] for m in trainers}
    i = 0
    for _ in range(a.rounds):
        for m, tr in trainers.items():
            for _ in range(a.warmup):
                tr.step(*data[i % 4])
                i += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step(*data[i % 4])
                i += 1
            torch.cuda.synchronize()
            rounds[m].append((time.perf_counter() - t0) / a.steps * 1e3)
    lines = [f"# tools/bench_modulation.py on {torch.cuda.get_device_name(dev)}: CREMA-D shapes, B = {B}, bf16, concat head, joint step,",
             f"# {a.rounds} rounds x ({a.warmup} warm-up + {a.steps} timed steps) per trainer, alternating; ms per step = median over the rounds",
             f"{'modulation':<12}{'ms':>9}{'vs Normal':>11}   rounds"]
    ms = {m: float(np.median(v)) for m, v in rounds.items()}
    for m, tr in trainers.items():
        try:  # (a run on random data may diverge: said in the table)
            r = tr.read()
            note = "" if np.isfinite(r["loss_f"]) else "   NOT FINITE"
            if "ogm" in r:
                note += "   last step: ratio_v %.3f coeff_a %.3f coeff_v %.3f" % (r["ogm"]["ratio_v"], r["ogm"]["coeff_a"], r["ogm"]["coeff_v"])
        except FloatingPointError:
            note = "   NOT FINITE"
        lines.append(f"{m:<12}{ms[m]:>9.3f}{ms[m] - ms['Normal']:>+11.3f}   " + " ".join(f"{x:.3f}" for x in rounds[m]) + note)
        tr.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
