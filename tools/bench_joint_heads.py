#!/usr/bin/env python3
"""Joint-training step against the DGL step without the early start, for each of the four fusion heads, on one MI355X.

    python tools/bench_joint_heads.py [--rounds 3] [--steps 100] [--warmup 20] [--out profiles/joint_heads_bench.txt]

CREMA-D shapes (spec 257 x 188, 3 frames of 224 x 224), B = 64, bf16 encoders.  Per head two trainers live in the process:
DGLTrainer(AVClassifier(args), mode="joint") -- one cross-entropy on the fused logits, the gradient through the head into both
encoders -- and DGLTrainer(AVClassifier_DGL(args), mode="dgl", early_backward=False) -- the DGL step in its junction form
(forward | head | backward), the form whose schedule the joint step shares.  They are timed alternately: per round and trainer
`warmup` untimed and `steps` timed steps between two device synchronisations (host clock), the median over the rounds is
reported.  Both trainers run without the visual engine's own weight-gradient side stream (as tools/bench_optimizers.py: two
owned side streams beside the chain streams and the caller's are more streams than hardware queues), so the two steps of a
head share one stream layout.  The joint step does strictly less head work (one logit set, one loss; FiLM: half the forward
contraction over fc.weight), so joint <= dgl is the expectation per head.
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

HEADS = ("concat", "sum", "gated", "film")


def build(fusion, joint, wl, batch, dev):
    """The model as main_dgl.py:230-246 builds it (seeded weight_init), with the joint or the DGL head of `fusion`."""
    from models.basic_model import AVClassifier, AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    setup_seed(0)
    args = argparse.Namespace(fusion_method=fusion, dataset=wl["dataset"], modality="full", batch_size=batch)
    model = (AVClassifier if joint else AVClassifier_DGL)(args)
    model.apply(weight_init)
    return model.to(dev).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", default=",".join(HEADS))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_joint_heads: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    wl, B = bench.WORKLOADS["cremad"], a.batch
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]
    lines = [f"# tools/bench_joint_heads.py on {torch.cuda.get_device_name(dev)}: CREMA-D shapes, B = {B}, bf16, "
             f"{a.rounds} rounds x ({a.warmup} warm-up + {a.steps} timed steps) per trainer, alternating joint / dgl;",
             "# ms per step = median over the rounds; dgl = mode=\"dgl\", early_backward=False; no visual side stream in either",
             f"{'head':<8}{'joint ms':>10}{'dgl(late) ms':>14}{'joint/dgl':>11}   rounds joint | dgl"]
    for fusion in a.heads.split(","):
        trainers = {
            "joint": DGLTrainer(build(fusion, True, wl, B, dev), lr=2e-3, max_norm=40.0, dtype="bf16", mode="joint",
                                visual_side_stream=False),
            "dgl": DGLTrainer(build(fusion, False, wl, B, dev), lr=2e-3, alpha=wl["alpha"], max_norm=40.0, dtype="bf16",
                              mode="dgl", early_backward=False, visual_side_stream=False),
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
        finite = {}
        for kind, tr in trainers.items():
            try:  # (a run on random data may diverge: said in the table, the timing of such a run is of no use)
                finite[kind] = bool(np.isfinite(tr.read()["loss_f"]))
            except FloatingPointError:
                finite[kind] = False
            tr.close()
        ms = {k: float(np.median(v)) for k, v in rounds.items()}
        fmt = lambda v: " ".join(f"{x:.3f}" for x in v)  # noqa: E731
        lines.append(f"{fusion:<8}{ms['joint']:>10.3f}{ms['dgl']:>14.3f}{ms['joint'] / ms['dgl']:>11.3f}   "
                     f"{fmt(rounds['joint'])} | {fmt(rounds['dgl'])}" + ("" if all(finite.values()) else f"   NOT FINITE: {finite}"))
        print(lines[-1], flush=True)
        del trainers, tr
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
