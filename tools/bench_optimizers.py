#!/usr/bin/env python3
"""The three optimizer updates of DGLTrainer(optimizer="sgd" | "Adam" | "AdaGrad") (main_dgl.py --optimizer), on one MI355X.

    python tools/bench_optimizers.py [--rounds 3] [--steps 100] [--warmup 20]

Prints ONE JSON line:
  kernels:  sgd_kernel / adamw_kernel / adagrad_kernel alone (nothing else on the device) over the flat arena of the B = 64
            CREMA-D ResNet18 pair (the trainer's `total`) and of the Swin-T composition, clip inactive and active.  Every
            kernel and regime starts from the same parameters and gradient and from zero state; the clip threshold is set from
            that gradient's norm right before the regime's grad_stats call (`clip_coef`: 1 = inactive, nothing written back;
            0.9995 = active, the clipped gradient written back by every launch).  20 warm-up and 200 timed launches between
            two device events; us per launch, algorithmic GB/s (20 / 28 / 20 bytes per element, the conditional gradient
            write-back not charged, as ProfScope charges them) and share of the 8 TB/s peak.
  step_ms:  the full step at bench.py's default workload (CREMA-D, B = 64, bf16, 4 resident batches) with each optimizer, one
            trainer per optimizer in this process, alternated: per round and optimizer 20 warm-up and 100 timed steps; the
            median over the rounds.  All three trainers run without the visual engine's own weight-gradient side stream
            (visual_side_stream=False): three owned side streams beside the two chain streams and the caller's are more
            streams than hardware queues (four): with them the second and third trainer built (Adam, AdaGrad) ran 0.76 /
            0.92 ms slower per step than the first, though the Adagrad update alone costs what SGD's does.  Without them no
            stream is created or destroyed while timing and the three steps share one stream layout; the optimizer update
            runs on the step's tail, behind the join of the chains, in either layout.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-gdl_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gdl.trainer import ADAGRAD_EPS, ADAM_BETAS, ADAM_EPS, DGLTrainer  # noqa: E402

HBM_PEAK_GBS = 8000.0
BYTES_PER_ELEMENT = {"sgd": 20, "adamw": 28, "adagrad": 20}


def time_kernels(tr, warmup=20, launches=200):
    """Each update kernel alone over arenas of the trainer's layout (its own descriptor), clip inactive / active."""
    dev, n = tr.device, tr.total
    g = torch.Generator(device=dev).manual_seed(5)
    P0 = torch.randn(n, device=dev, generator=g)
    G0 = torch.randn(n, device=dev, generator=g) * 1e-3
    P, G = torch.empty_like(P0), torch.empty_like(G0)
    S1, S2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    stats = torch.zeros_like(tr.stats)
    st = L.cur_stream()
    out = {}
    for kernel in ("sgd", "adamw", "adagrad"):
        def launch(t):
            if kernel == "sgd":
                L.call("gdl_optim_sgd_step", tr.opt, L.ptr(P), L.ptr(G), L.ptr(S1), L.ptr(stats), 1.0, 2e-3, 0.9, 1e-4, st)
            elif kernel == "adamw":
                L.call("gdl_optim_adamw_step", tr.opt, L.ptr(P), L.ptr(G), L.ptr(S1), L.ptr(S2), L.ptr(stats), 1.0, 2e-3,
                       ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, 1e-2, t, st)
            else:
                L.call("gdl_optim_adagrad_step", tr.opt, L.ptr(P), L.ptr(G), L.ptr(S1), L.ptr(stats), 1.0, 2e-3, ADAGRAD_EPS,
                       0.0, t, st)

        res = {}
        for clip in ("clip_off", "clip_on"):
            # the same start for every kernel and regime (an active clip's write-back shrinks G launch by launch)
            P.copy_(P0)
            G.copy_(G0)
            S1.zero_()
            S2.zero_()
            norm = float(G.double().norm())
            # inactive: coefficient 1, the gradient is not written back; active: coefficient 0.9995, written back each launch
            max_norm = 1e30 if clip == "clip_off" else 0.9995 * norm
            L.call("gdl_optim_grad_stats", tr.opt, L.ptr(G), max_norm, 1.0, L.ptr(stats), L.ptr(tr.opt_ws), tr.opt_ws_bytes, st)
            coef = float(stats[1].item())
            assert (coef == 1.0) if clip == "clip_off" else (coef < 1.0), (kernel, clip, coef)
            for t in range(1, warmup + 1):
                launch(t)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in range(warmup + 1, warmup + launches + 1):
                launch(t)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / launches
            gbs = n * BYTES_PER_ELEMENT[kernel] / us / 1e3
            res[clip] = {"us": round(us, 2), "gbs": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 3),
                         "clip_coef": round(coef, 6)}
        out[kernel] = res
    del P, G, P0, G0, S1, S2
    return {"total": n, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    kernels = {}
    for key, wl in (("resnet18_cremad", bench.WORKLOADS["cremad"]), ("swin_t_vggsound", bench.WORKLOADS["vggsound_swin"])):
        model, _ = bench.build_model(wl, a.batch, dev)
        tr = DGLTrainer(model, lr=2e-3, alpha=wl["alpha"], max_norm=40.0, dtype="bf16")  # (no step: the arenas only)
        kernels[key] = time_kernels(tr)
        tr.close()
        del tr, model
        torch.cuda.empty_cache()
    wl = bench.WORKLOADS["cremad"]
    B = a.batch
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]
    trainers = {}
    for kind in ("sgd", "Adam", "AdaGrad"):
        model, _ = bench.build_model(wl, B, dev)
        trainers[kind] = DGLTrainer(model, lr=2e-3, alpha=wl["alpha"], max_norm=40.0, dtype="bf16", optimizer=kind,
                                    visual_side_stream=False)
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
            rounds[kind].append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
    assert not any(tr.eng_v.has_side_stream() for tr in trainers.values())
    step_ms = {k: float(np.median(v)) for k, v in rounds.items()}
    finite = {k: bool(np.isfinite(tr.read()["loss_f"])) for k, tr in trainers.items()}
    r = kernels["resnet18_cremad"]
    out = {"device": torch.cuda.get_device_name(dev), "batch": B, "dtype": "bf16", "kernels": kernels,
           "kernel_ratio_vs_sgd": {k: {c: round(r[k][c]["us"] / r["sgd"][c]["us"], 3) for c in ("clip_off", "clip_on")}
                                   for k in ("adamw", "adagrad")},
           "step_ms": step_ms, "step_ms_rounds": rounds,
           "step_delta_ms_vs_sgd": {k: round(step_ms[k] - step_ms["sgd"], 4) for k in ("Adam", "AdaGrad")},
           "step_schedule": "visual_side_stream=False for all three trainers", "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "losses_finite": finite}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
