#!/usr/bin/env python3
"""The feature-diversity monitor (csrc/diversity.hip) alone and inside the B = 64 CREMA-D DGL step, on one MI355X.

    python tools/bench_diversity.py [--rounds 5] [--steps 100] [--warmup 20] [--out profiles/diversity_bench.txt]

1. The kernel alone through gdl_feature_diversity at the shapes a step launches it with -- (192, 49) the CREMA-D visual map,
   (64, 54) its audio map, (64, 100) the Kinetics-Sounds audio map -- NHWC, bf16 and float32: back-to-back launches between two
   device events, us per launch and the achieved GB/s against the bytes it must read once (n_img P 512 elements).
2. The DGL step (concat head, bf16, spec 257 x 188, 3 frames of 224 x 224, synthetic batches) with the switch off and on: FOUR
   trainers in one process, two of each kind, timed alternately (per round and trainer `warmup` untimed and `steps` timed steps
   between two device synchronisations, host clock; median over the rounds).  The difference between the two trainers of ONE
   kind is the run's own spread -- the yardstick profiles/ablation_bench.txt uses; the on/off difference is read against it.
   The `off` trainers are THIS commit's step with the switch off, not a timing of the parent commit: off, the switch adds one
   host-side `if` per forward, no launch and no allocation -- an argument, not a measurement.  The parent's step is measured
   by `bench.py --gpus 1` on a checkout of the parent, beside the same command here (the flagship step never turns the
   switch on).
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


def build(wl, batch, dev):
    """The model as main_dgl.py:230-246 builds it (seeded weight_init)."""
    from models.basic_model import AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    setup_seed(0)
    model = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset=wl["dataset"], modality="full", batch_size=batch))
    model.apply(weight_init)
    return model.to(dev).train()


def bench_kernel(a, dev, lines):
    lines.append(f"{'kernel alone: (n_img, P), dtype':<36}{'us min':>8}{'median':>8}{'max':>8}{'MB read':>9}{'GB/s':>8}")
    st = L.cur_stream()
    for dt_name, tdt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        for n, P in ((192, 49), (64, 54), (64, 100)):
            gen = torch.Generator(device=dev).manual_seed(n * 1000 + P)
            x = torch.randn(n, P, 512, generator=gen, device=dev).clamp_min(0).to(tdt)
            ws = torch.zeros(L.load().gdl_feature_diversity_workspace_bytes(n), dtype=torch.uint8, device=dev)
            mean, acc = torch.zeros(1, device=dev), torch.zeros(2, device=dev)

            def fn():
                L.call("gdl_feature_diversity", L.ptr(x), L.dtype_code(dt_name), L.GDL_LAYOUT_NHWC, n, P, 512, None, L.ptr(mean),
                       L.ptr(acc), L.ptr(ws), ws.numel(), st)

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
            mb = x.numel() * x.element_size() / 1e6
            med = float(np.median(us))
            lines.append(f"{'(' + str(n) + ', ' + str(P) + '), ' + dt_name:<36}{min(us):>8.2f}{med:>8.2f}{max(us):>8.2f}{mb:>9.2f}"
                         f"{mb / med * 1e3:>8.0f}")
            print(lines[-1], flush=True)
            assert bool(torch.isfinite(mean).all())


def bench_steps(a, dev, lines):
    wl, B = bench.WORKLOADS["cremad"], a.batch
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]
    kw = dict(lr=2e-3, max_norm=40.0, dtype="bf16", alpha=wl["alpha"])
    trainers = {f"{name} {tag}": DGLTrainer(build(wl, B, dev), diversity=on, **kw)
                for tag in ("A", "B") for name, on in (("off", False), ("on", True))}
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
    ms = {k: float(np.median(v)) for k, v in rounds.items()}
    lines.append(f"{'DGL step, diversity':<22}{'ms':>8}   rounds")
    for kind, tr in trainers.items():
        extra = ""
        if kind.startswith("on"):
            ep = tr.epoch_diversity()
            extra = f"   epoch means a {ep['a_diversity']:.4f} v {ep['v_diversity']:.4f}"
        tr.close()
        lines.append(f"{kind:<22}{ms[kind]:>8.3f}   " + " ".join(f"{x:.3f}" for x in rounds[kind]) + extra)
        print(lines[-1], flush=True)
    off, on = (ms["off A"] + ms["off B"]) / 2, (ms["on A"] + ms["on B"]) / 2
    spread = max(abs(ms["off A"] - ms["off B"]), abs(ms["on A"] - ms["on B"]))
    lines.append(f"# on - off = {on - off:+.4f} ms ({(on - off) / off * 100:+.2f} %); spread between two trainers of one kind = "
                 f"{spread:.4f} ms: the switch {'EXCEEDS' if on - off > spread else 'is within'} the run's own spread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_diversity: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    lines = [f"# tools/bench_diversity.py on {torch.cuda.get_device_name(dev)}",
             f"# 1. gdl_feature_diversity alone, NHWC: {a.repeats} repeats x {a.launches} back-to-back launches, us per launch "
             "(device events); GB/s = the map's bytes, read once, over the median"]
    bench_kernel(a, dev, lines)
    lines += ["#", f"# 2. the DGL step, CREMA-D shapes, B = {a.batch}, bf16, concat head: {a.rounds} rounds x ({a.warmup} warm-up + "
              f"{a.steps} timed steps) per trainer, the four alternating; ms per step = median over the rounds.",
              "#    off = this commit, diversity=False (no launch, nothing allocated; NOT a timing of the parent commit: that is "
              "bench.py's, on a checkout of the parent);",
              "#    on = one gdl_encoder_feature_diversity behind each encoder's forward, on its chain"]
    bench_steps(a, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
