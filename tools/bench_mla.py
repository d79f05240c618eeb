#!/usr/bin/env python3
"""Alternating unimodal training on a shared head (csrc/mla.hip, gdl.MLATrainer) alone and as a step, on one MI355X.

    python tools/bench_mla.py [--rounds 5] [--steps 100] [--warmup 20] [--parent-tree DIR] [--out profiles/mla_bench.txt]

1. The new launches alone, back-to-back between two device events, us per launch: gdl_mla_feature_mean at B = 64,
   gdl_mla_projector_update with and without the normalisation (P re-seeded with the identity every window), gdl_mla_project
   and gdl_mla_fuse (B = 64, entropy weights) at n = 6 (CREMA-D), 34 (Kinetics-Sounds) and 309 (VGGSound) classes.
2. The step (bf16, spec 257 x 188, 3 frames of 224 x 224, B = 64, synthetic batches), three settings alternating in one process,
   the order rotated from round to round: ONE MLATrainer with shaping on, the same trainer with shaping off, and the parent
   commit's way to run the same work -- one UnimodalTrainer audio step followed by one UnimodalTrainer visual step (two models:
   the heads are not shared there, the launches are the same).  Per round and setting `warmup` untimed and `steps` timed steps,
   host clock around the steps and one device synchronisation; medians over the rounds with the lowest and the highest.
3. With --parent-tree (a checkout of the parent commit, built): `bench.py --gpus 1` (the flagship DGL step; the new code is not
   on its path) there and here, alternating, a fresh process each -- run BEFORE this process touches the device.
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
        raise SystemExit(f"bench_mla: bench.py in {tree} ended with {p.returncode}:\n{p.stderr[-2000:]}")
    return float(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])


def _med(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else (v[len(v) // 2 - 1] + v[len(v) // 2]) / 2


def bench_parent(a, lines):
    here, parent = [], []
    for k in range(a.pairs):  # (the order within a pair alternates: neither tree always runs on the warmer device)
        for tree in ((a.parent_tree, ROOT) if k % 2 == 0 else (ROOT, a.parent_tree)):
            (here if tree == ROOT else parent).append(bench_py(tree, a))
        print(f"bench.py: parent {parent[-1]:.3f} ms, this tree {here[-1]:.3f} ms", flush=True)
    sp = max(max(parent) - min(parent), max(here) - min(here))
    d = _med(here) - _med(parent)
    lines += ["parent commit     " + " ".join(f"{x:8.3f}" for x in parent) + f"   median {_med(parent):.3f}",
              "this commit       " + " ".join(f"{x:8.3f}" for x in here) + f"   median {_med(here):.3f}",
              f"# this - parent (medians) = {d:+.4f} ms; spread between the runs of one tree = {sp:.4f} ms: the default step "
              f"{'DIFFERS BY MORE THAN' if abs(d) > sp else 'lies within'} the job's own spread"]


def timed(fn, a, before=None):
    """us per launch of fn: (min, median, max) over a.repeats windows of a.launches back-to-back launches"""
    import torch

    us = []
    for _ in range(a.repeats):
        for _ in range(20):
            fn()
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) / a.launches * 1e3)
    return min(us), _med(us), max(us)


def bench_kernels(a, dev, lines):
    import torch

    from gdl import _lib as L

    st = L.cur_stream()
    B = a.batch
    g = torch.Generator(device="cpu").manual_seed(7)
    h = torch.randn(B, 512, generator=g).clamp_min(0).to(dev)
    r = h.mean(dim=0)
    eye = torch.eye(512, device=dev)
    P = eye.clone()
    ws = torch.empty(L.load().gdl_mla_projector_workspace_bytes(), dtype=torch.uint8, device=dev)
    rows = [(f"gdl_mla_feature_mean B={B}", lambda: L.call("gdl_mla_feature_mean", h.data_ptr(), B, r.data_ptr(), st), None)]
    for norm in (1, 0):
        # (without the normalisation P shrinks towards 0 along r over a window; the launches' work does not depend on the values)
        rows.append((f"gdl_mla_projector_update normalize={norm}",
                     lambda norm=norm: L.call("gdl_mla_projector_update", P.data_ptr(), r.data_ptr(), 0.1, norm, ws.data_ptr(),
                                              ws.numel(), st), lambda: P.copy_(eye)))
    P3 = eye.clone()
    for i in range(3):
        L.call("gdl_mla_projector_update", P3.data_ptr(), h[i * 8:(i + 1) * 8].mean(dim=0).data_ptr(), 0.1, 1, ws.data_ptr(), ws.numel(), st)
    for n in (6, 34, 309):
        dW0 = (torch.randn(n, 512, generator=g) / 64).to(dev)
        dW = dW0.clone()
        oa, ov = (2 * torch.randn(B, n, generator=g)).to(dev), (3 * torch.randn(B, n, generator=g)).to(dev)
        out, lam = torch.empty((B, n), device=dev), torch.empty((B, 2), device=dev)
        # (dW P^T in place with ||P||_F = 1 decays towards 0 over a window: re-seeded in front of every window)
        rows.append((f"gdl_mla_project  n={n}", lambda dW=dW, n=n: L.call("gdl_mla_project", dW.data_ptr(), P3.data_ptr(), n, st),
                     lambda dW=dW, dW0=dW0: dW.copy_(dW0)))
        rows.append((f"gdl_mla_fuse     B={B} n={n}",
                     lambda oa=oa, ov=ov, out=out, lam=lam, n=n: L.call("gdl_mla_fuse", oa.data_ptr(), ov.data_ptr(), B, n, 1,
                                                                        out.data_ptr(), lam.data_ptr(), st), None))
    lines.append(f"{'launch alone':<44}{'us min':>9}{'median':>9}{'max':>9}")
    for name, fn, before in rows:
        lo, med, hi = timed(fn, a, before)
        lines.append(f"{name:<44}{lo:>9.2f}{med:>9.2f}{hi:>9.2f}")
        print(lines[-1], flush=True)


def bench_step(a, dev, lines):
    import torch

    import bench
    from gdl.mla import MLATrainer
    from gdl.unimodal import UnimodalTrainer
    from models.basic_model import AVClassifier_DGL, AVClassifier_MLA
    from utils.utils import setup_seed, weight_init

    wl, B = bench.WORKLOADS["cremad"], a.batch
    n = wl["n_classes"]

    def make(cls, modality):
        setup_seed(0)
        m = cls(argparse.Namespace(fusion_method="concat", dataset=wl["dataset"], modality=modality, batch_size=B))
        m.apply(weight_init)
        return m.to(dev).train()

    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, n, (B,), generator=g).to(dev)) for _ in range(4)]
    mla = MLATrainer(make(AVClassifier_MLA, "full"), lr=2e-3, dtype="bf16")
    ua = UnimodalTrainer(make(AVClassifier_DGL, "audio"), lr=2e-3, dtype="bf16")
    uv = UnimodalTrainer(make(AVClassifier_DGL, "visual"), lr=2e-3, dtype="bf16")

    def step_mla(d):
        mla.step(*d)

    def step_uni(d):
        ua.step(d[0], None, d[2])
        uv.step(None, d[1], d[2])

    kinds = ["mla_on", "mla_off", "unimodal"]
    t = {k: [] for k in kinds}
    i = 0
    for r in range(a.rounds):
        for k in kinds[r % 3:] + kinds[:r % 3]:
            mla.shaping = k == "mla_on"
            fn = step_uni if k == "unimodal" else step_mla
            for _ in range(a.warmup):
                fn(data[i % 4])
                i += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn(data[i % 4])
                i += 1
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        print("round", r, {k: round(v[-1], 3) for k, v in t.items()}, flush=True)
    r = mla.read()
    assert all(x == x for x in (r["loss_a"], r["loss_v"])), "the MLA run diverged"
    for tr in (mla, ua, uv):
        tr.close()
    label = {"mla_on": "MLATrainer.step, shaping on", "mla_off": "MLATrainer.step, shaping off",
             "unimodal": "UnimodalTrainer audio + visual"}
    lines.append(f"{'one batch':<34}{'ms median':>10}{'min':>8}{'max':>8}   rounds")
    for k in kinds:
        lines.append(f"{label[k]:<34}{_med(t[k]):>10.3f}{min(t[k]):>8.3f}{max(t[k]):>8.3f}   " + " ".join(f"{x:.3f}" for x in t[k]))
    floor = max(max(v) - min(v) for v in t.values())
    for k in ("mla_on", "mla_off"):
        d = _med(t[k]) - _med(t["unimodal"])
        lines.append(f"# {label[k]} - the unimodal sequence (medians) = {d:+.4f} ms ({d / _med(t['unimodal']) * 100:+.2f} %); largest "
                     f"spread between rounds of one setting = {floor:.4f} ms: the difference "
                     f"{'EXCEEDS' if abs(d) > floor else 'is not resolved by'} it")
    d = _med(t["mla_on"]) - _med(t["mla_off"])
    lines.append(f"# shaping on - off (medians) = {d:+.4f} ms: {'EXCEEDS' if abs(d) > floor else 'not resolved by'} the spread")
    print("\n".join(lines[-7:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=500)
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
        raise SystemExit("bench_mla: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    lines = [f"# tools/bench_mla.py on {torch.cuda.get_device_name(dev)}",
             f"# 1. the new launches alone: {a.repeats} repeats x {a.launches} back-to-back launches, us per launch (device events); "
             "gdl_mla_projector_update is two launches, three with the normalisation"]
    bench_kernels(a, dev, lines)
    lines += ["#", f"# 2. one batch, CREMA-D shapes, B = {a.batch}, bf16: {a.rounds} rounds x ({a.warmup} warm-up + {a.steps} timed steps) "
              "per setting, alternating in one process, the order rotated every round; ms per batch (host clock, one synchronisation)"]
    bench_step(a, dev, lines)
    if parent_lines:
        lines += ["#", f"# 3. bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup} --no-extra --no-comparator --no-f32 (the flagship DGL "
                  "step; the new code is not on its path) on a checkout of the parent commit and on this commit, alternating in one job "
                  "on the same device, a process each, before section 1; ms per step"] + parent_lines
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
