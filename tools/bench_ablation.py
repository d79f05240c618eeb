#!/usr/bin/env python3
"""The multi-task baseline's step (DGLTrainer, detach_fused=False, drop_head_uni=False) beside the DGL step and the joint step, with
the fused junction (gdl_head_mtl_ce) and with the three launches it replaces, on one MI355X.

    python tools/bench_ablation.py [--rounds 3] [--steps 100] [--warmup 20] [--out profiles/ablation_bench.txt]

CREMA-D shapes (spec 257 x 188, 3 frames of 224 x 224), B = 64, bf16 encoders, synthetic batches.  Six trainers live in the
process and are timed alternately: per round and trainer `warmup` untimed and `steps` timed steps between two device
synchronisations (host clock); the median over the rounds is reported.
  dgl concat             the DGL step (early backward: no junction)
  joint concat           mode="joint": one loss, the junction form with gdl_head_concat_fwd + gdl_softmax_ce + dx / dy
  mtl concat / sum       the multi-task step, gdl_head_mtl_ce at the junction
  mtl concat / sum 3x    the same with the three-launch junction (the tuning aid GDL_TUNING=1 GDL_MTL_FUSED=0, which DGLTrainer
                         reads when it is constructed: set around the construction of these two trainers only)
All without the visual engine's own weight-gradient side stream (as tools/bench_joint_heads.py), so every step has one stream
layout.  Then the two junctions alone, as tools/bench_unimodal.py times its launches: back-to-back junctions between two device
events, us per junction.
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


def build(fusion, joint, wl, batch, dev):
    """The model as main_dgl.py:230-246 builds it (seeded weight_init)."""
    from models.basic_model import AVClassifier, AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    setup_seed(0)
    args = argparse.Namespace(fusion_method=fusion, dataset=wl["dataset"], modality="full", batch_size=batch)
    model = (AVClassifier if joint else AVClassifier_DGL)(args)
    model.apply(weight_init)
    return model.to(dev).train()


def three_launch_trainer(*args, **kw):
    """A trainer whose junction is the three launches: the tuning aid is in the environment while the constructor reads it."""
    saved = {k: os.environ.get(k) for k in ("GDL_TUNING", "GDL_MTL_FUSED")}
    os.environ.update(GDL_TUNING="1", GDL_MTL_FUSED="0")
    try:
        tr = DGLTrainer(*args, **kw)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert not tr.mtl_fused
    return tr


def bench_steps(a, dev, lines):
    wl, B = bench.WORKLOADS["cremad"], a.batch
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]
    kw = dict(lr=2e-3, max_norm=40.0, dtype="bf16", visual_side_stream=False)
    mtl = dict(kw, alpha=2.5, detach_fused=False, drop_head_uni=False)
    trainers = {
        "dgl concat": DGLTrainer(build("concat", False, wl, B, dev), alpha=wl["alpha"], **kw),
        "joint concat": DGLTrainer(build("concat", True, wl, B, dev), mode="joint", **kw),
        "mtl concat": DGLTrainer(build("concat", False, wl, B, dev), **mtl),
        "mtl concat 3x": three_launch_trainer(build("concat", False, wl, B, dev), **mtl),
        "mtl sum": DGLTrainer(build("sum", False, wl, B, dev), **mtl),
        "mtl sum 3x": three_launch_trainer(build("sum", False, wl, B, dev), **mtl),
    }
    assert trainers["mtl concat"].mtl_fused and trainers["mtl sum"].mtl_fused
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
    lines.append(f"{'step':<16}{'ms':>8}{'of joint':>10}   rounds")
    ms = {k: float(np.median(v)) for k, v in rounds.items()}
    for kind, tr in trainers.items():
        try:  # (a run on random data may diverge: said in the table, the timing of such a run is of no use)
            finite = bool(np.isfinite(tr.read()["loss_f"]))
        except FloatingPointError:
            finite = False
        tr.close()
        lines.append(f"{kind:<16}{ms[kind]:>8.3f}{ms[kind] / ms['joint concat']:>10.3f}   " + " ".join(f"{x:.3f}" for x in rounds[kind])
                     + ("" if finite else "   NOT FINITE"))
        print(lines[-1], flush=True)
    for head in ("concat", "sum"):
        f, t = rounds[f"mtl {head}"], rounds[f"mtl {head} 3x"]
        lines.append(f"# mtl {head}: fused / three-launch = {ms[f'mtl {head}'] / ms[f'mtl {head} 3x']:.4f} (medians); every fused round "
                     f"<= every three-launch round: {'yes' if max(f) <= min(t) else 'no'}")


def bench_junctions(a, dev, lines):
    B, alpha = a.batch, 2.5
    lines.append(f"{'junction, head, (B, n)':<44}{'us min':>8}{'median':>8}{'max':>8}")
    for head in ("concat", "sum"):
        for n in (6, 309):
            gen = torch.Generator(device=dev).manual_seed(n)
            fa = torch.randn(B, 512, generator=gen, device=dev).clamp_min(0)
            fv = torch.randn(B, 512, generator=gen, device=dev).clamp_min(0)
            lab = torch.randint(0, n, (B,), generator=gen, device=dev)
            if head == "concat":
                W, b = torch.randn(n, 1024, generator=gen, device=dev) * 0.02, torch.randn(n, generator=gen, device=dev) * 0.1
                wargs = (L.ptr(W), W.data_ptr() + 512 * 4, 1024, L.ptr(b), L.ptr(b), 0)
            else:
                Wx, Wy = (torch.randn(n, 512, generator=gen, device=dev) * 0.02 for _ in range(2))
                bx, by = (torch.randn(n, generator=gen, device=dev) * 0.1 for _ in range(2))
                wargs = (L.ptr(Wx), L.ptr(Wy), 512, L.ptr(bx), L.ptr(by), 1)
            out, oa, ov, gf, ga, gv = (torch.empty(B, n, device=dev) for _ in range(6))
            dfa, dfv, losses = torch.empty(B, 512, device=dev), torch.empty(B, 512, device=dev), torch.empty(3, device=dev)
            ws = torch.zeros(L.load().gdl_head_mtl_ce_workspace_bytes(B), dtype=torch.uint8, device=dev)
            st = L.cur_stream()

            def fused():
                L.call("gdl_head_mtl_ce", L.ptr(fa), L.ptr(fv), *wargs, L.ptr(lab), alpha, 1, L.ptr(out), L.ptr(oa), L.ptr(ov),
                       L.ptr(losses), L.ptr(gf), L.ptr(ga), L.ptr(gv), L.ptr(dfa), L.ptr(dfv), B, n, L.ptr(ws), ws.numel(), st)

            def three():
                if head == "concat":
                    L.call("gdl_head_concat_fwd", L.ptr(fa), L.ptr(fv), L.ptr(W), L.ptr(b), L.ptr(out), L.ptr(oa), L.ptr(ov), B, n, st)
                else:
                    L.call("gdl_head_sum_fwd", L.ptr(fa), L.ptr(fv), L.ptr(Wx), L.ptr(bx), L.ptr(Wy), L.ptr(by), L.ptr(out), L.ptr(oa),
                           L.ptr(ov), B, n, st)
                L.call("gdl_softmax_ce3", L.ptr(out), L.ptr(oa), L.ptr(ov), L.ptr(lab), 1.0, alpha, alpha, L.ptr(losses), L.ptr(gf),
                       L.ptr(ga), L.ptr(gv), B, n, st)
                if head == "concat":
                    L.call("gdl_head_concat_bwd", L.ptr(fa), L.ptr(fv), L.ptr(W), L.ptr(ga), L.ptr(gv), L.ptr(gf), 1, 0, L.ptr(dfa),
                           L.ptr(dfv), None, None, B, n, st)
                else:
                    L.call("gdl_head_sum_bwd", L.ptr(fa), L.ptr(fv), L.ptr(Wx), L.ptr(Wy), L.ptr(ga), L.ptr(gv), L.ptr(gf), 1, 0,
                           L.ptr(dfa), L.ptr(dfv), None, None, None, None, B, n, st)

            calls = {"gdl_head_mtl_ce": fused, "fwd + ce3 + bwd(dx, dy)": three}
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
                lines.append(f"{k + ', ' + head + ', (' + str(B) + ', ' + str(n) + ')':<44}{min(v):>8.2f}{float(np.median(v)):>8.2f}{max(v):>8.2f}")
                print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ablation: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    lines = [f"# tools/bench_ablation.py on {torch.cuda.get_device_name(dev)}: CREMA-D shapes, B = {a.batch}, bf16, "
             f"{a.rounds} rounds x ({a.warmup} warm-up + {a.steps} timed steps) per trainer, the six alternating;",
             "# ms per step = median over the rounds; mtl = detach_fused=False, drop_head_uni=False, alpha 2.5; 3x = the three-launch "
             "junction; no visual side stream anywhere"]
    bench_steps(a, dev, lines)
    torch.cuda.empty_cache()
    lines += ["#", f"# the junction alone, fused_reaches = 1: {a.repeats} repeats x {a.launches} back-to-back junctions, alternating; "
              "us per junction (device events)"]
    bench_junctions(a, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
