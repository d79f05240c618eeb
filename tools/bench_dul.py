#!/usr/bin/env python3
"""The probabilistic-embedding branch (csrc/dul.hip, gdl/dul.py) alone and inside the B = 64 CREMA-D steps, on one MI355X.

    python tools/bench_dul.py [--rounds 5] [--steps 60] [--warmup 15] [--parent-tree DIR] [--out profiles/dul_bench.txt]

1. The four launches alone, back-to-back between two device events, us per launch, bf16, B = 64: the audio maps of CREMA-D
   (M = 64 x 54) and Kinetics-Sounds (M = 64 x 100) and the visual map (M = 192 x 49, T = 3); gdl_dul_eval at B = 64.
2. The joint concat step and the multi-task concat step (mode="dgl", detach_fused=False, drop_head_uni=False) at the CREMA-D
   shapes (bf16, spec 257 x 188, 3 frames of 224 x 224, synthetic batches): a trainer on a model WITH the stacks (beta 1e-5)
   against the same trainer class on a model without them, alternating windows in one process, the order swapped from round to
   round; the spread between rounds of one setting is the noise floor.
3. With --parent-tree (a checkout of the parent commit, built): `bench.py --gpus 1` (the flagship DGL step, which the branch is
   not on) there and here, alternating, a fresh process each -- run BEFORE this process touches the device.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-gdl_amd"), os.path.join(ROOT, "tools")]

import bench_pmr as bp  # noqa: E402  (bench_py / bench_parent / timed: the same protocol)


def bench_kernels(a, dev, lines):
    import torch

    from gdl import _lib as L

    lib, st, dt = L.load(), L.cur_stream(), L.GDL_BF16
    g = torch.Generator(device="cpu").manual_seed(7)
    lines.append(f"{'launch alone (bf16)':<44}{'us min':>9}{'median':>9}{'max':>9}")
    for name, n_img, T, P in (("audio CREMA-D  M=64x54", 64, 1, 54), ("audio KS       M=64x100", 64, 1, 100), ("visual        M=192x49", 192, 3, 49)):
        M, B = n_img * P, n_img // T
        z = [torch.randn(M, 512, generator=g).to(dev).bfloat16() for _ in range(2)]
        bn = [torch.stack([1 + 0.1 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g),
                           0.5 + torch.rand(512, generator=g)]).to(dev) for _ in range(2)]
        gam = [torch.ones(512, device=dev) for _ in range(2)]
        f, reg, df = torch.empty(B, 512, device=dev), torch.empty(1, device=dev), torch.randn(B, 512, generator=g).to(dev)
        nb = lib.gdl_dul_sample_workspace_bytes(dt, n_img, T)
        ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
        blocks = lib.gdl_bn_bwd_blocks(M, 512)
        part = [torch.empty(blocks, 512, 2, device=dev) for _ in range(2)]
        coef = [torch.zeros(2, 512, device=dev) for _ in range(2)]
        dz = [torch.empty_like(z[0]) for _ in range(2)]

        def sample():
            L.call("gdl_dul_sample", dt, L.ptr(z[0]), L.ptr(z[1]), L.ptr(bn[0]), L.ptr(bn[1]), None, 1, 2, 0, L.ptr(f), L.ptr(reg), None, None,
                   None, None, n_img, T, P, 512, L.ptr(ws), nb, st)

        def reduce_():
            L.call("gdl_dul_bwd_reduce", dt, L.ptr(z[0]), L.ptr(z[1]), L.ptr(df), None, 1, 2, 0, 1e-5, L.ptr(bn[0]), L.ptr(bn[1]),
                   L.ptr(part[0]), L.ptr(part[1]), n_img, T, P, 512, st)

        def apply_():
            L.call("gdl_dul_bwd_apply", dt, L.ptr(z[0]), L.ptr(z[1]), L.ptr(df), None, 1, 2, 0, 1e-5, L.ptr(bn[0]), L.ptr(bn[1]), L.ptr(gam[0]),
                   L.ptr(gam[1]), L.ptr(coef[0]), L.ptr(coef[1]), L.ptr(dz[0]), L.ptr(dz[1]), n_img, T, P, 512, st)

        for kn, fn in (("gdl_dul_sample", sample), ("gdl_dul_bwd_reduce", reduce_), ("gdl_dul_bwd_apply", apply_)):
            lo, med, hi = bp.timed(fn, a)
            lines.append(f"{kn + '  ' + name:<44}{lo:>9.2f}{med:>9.2f}{hi:>9.2f}")
            print(lines[-1], flush=True)
    fe, W, b = torch.randn(64, 512, generator=g).to(dev), (0.05 * torch.randn(512, 512, generator=g)).to(dev), torch.zeros(512, device=dev)
    sc, out = torch.ones(512, device=dev), torch.empty(64, 512, device=dev)
    lo, med, hi = bp.timed(lambda: L.call("gdl_dul_eval", L.ptr(fe), L.ptr(W), L.ptr(b), L.ptr(sc), L.ptr(b), L.ptr(out), 64, 512, st), a)
    lines.append(f"{'gdl_dul_eval  B=64':<44}{lo:>9.2f}{med:>9.2f}{hi:>9.2f}")
    print(lines[-1], flush=True)


def bench_step(a, dev, lines, mode):
    import numpy as np
    import torch

    import bench
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier, AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    wl, B = bench.WORKLOADS["cremad"], a.batch
    n = wl["n_classes"]
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, n, (B,), generator=g).to(dev)) for _ in range(4)]
    tr = {}
    for pe in (0, 1):
        setup_seed(0)
        args = argparse.Namespace(fusion_method="concat", dataset=wl["dataset"], modality="full", batch_size=B, pe=pe)
        model = (AVClassifier if mode == "joint" else AVClassifier_DGL)(args)
        model.apply(weight_init)
        model = model.to(dev).train()
        kw = dict(mode="joint") if mode == "joint" else dict(mode="dgl", alpha=2.5, detach_fused=False, drop_head_uni=False)
        tr[pe] = DGLTrainer(model, lr=2e-3, max_norm=40.0, dtype="bf16", beta=1e-5 if pe else 0.0, **kw)
    t = {0: [], 1: []}
    i = 0
    for r in range(a.rounds):
        for pe in ((0, 1) if r % 2 == 0 else (1, 0)):
            for _ in range(a.warmup):
                tr[pe].step(*data[i % 4])
                i += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr[pe].step(*data[i % 4])
                i += 1
            torch.cuda.synchronize()
            t[pe].append((time.perf_counter() - t0) / a.steps * 1e3)
    assert "regurize_a" in tr[1].read() and "regurize_a" not in tr[0].read()
    for x in tr.values():
        x.close()
    off, on = float(np.median(t[0])), float(np.median(t[1]))
    floor = max(max(t[0]) - min(t[0]), max(t[1]) - min(t[1]))
    lines += [f"{mode + ' concat step':<26}{'ms median':>10}{'min':>8}{'max':>8}   rounds",
              f"{'without the branch':<26}{off:>10.3f}{min(t[0]):>8.3f}{max(t[0]):>8.3f}   " + " ".join(f"{x:.3f}" for x in t[0]),
              f"{'with it (beta 1e-5)':<26}{on:>10.3f}{min(t[1]):>8.3f}{max(t[1]):>8.3f}   " + " ".join(f"{x:.3f}" for x in t[1]),
              f"# with - without (medians) = {on - off:+.4f} ms ({(on - off) / off * 100:+.2f} %); spread between rounds of one setting = "
              f"{floor:.4f} ms: the difference {'EXCEEDS it' if on - off > floor else 'is not resolved'}"]
    print("\n".join(lines[-4:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: bench.py there and here (section 3)")
    ap.add_argument("--pairs", type=int, default=3, help="bench.py runs per tree in section 3")
    ap.add_argument("--out", default="")
    ap.add_argument("--digest", default="", help="a built checkout (e.g. the parent commit): print tests/test_dul_gpu.py's "
                    "pe_off_digest of both runners computed with THAT tree's library and Python, as JSON, and exit")
    a = ap.parse_args()
    if a.digest:  # what tests/golden/dul_pe_off_parent.json records
        import json
        import subprocess

        tree = os.path.abspath(a.digest)
        code = ("import importlib.util, json; s = importlib.util.spec_from_file_location('t', %r); m = importlib.util.module_from_spec(s); "
                "s.loader.exec_module(m); print(json.dumps({k: m.pe_off_digest(k)[0] for k in ('unimodal', 'joint')}))"
                % os.path.join(ROOT, "tests", "test_dul_gpu.py"))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([tree, os.path.join(tree, "iccv2025-gdl_amd"), os.path.join(ROOT, "tests")]))
        env.pop("GDL_LIB", None)
        p = subprocess.run([sys.executable, "-c", code], cwd=tree, env=env, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise SystemExit(f"bench_dul --digest: ended with {p.returncode}:\n{p.stderr[-3000:]}")
        print(p.stdout.strip().splitlines()[-1])
        return
    parent_lines = []
    if a.parent_tree:  # fresh processes, before this one opens the device
        bp.bench_parent(a, parent_lines)
    import torch

    from gdl import _lib as L

    if not torch.cuda.is_available():
        raise SystemExit("bench_dul: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    lines = [f"# tools/bench_dul.py on {torch.cuda.get_device_name(dev)}",
             f"# 1. the four launches alone: {a.repeats} repeats x {a.launches} back-to-back launches, us per launch (device events); one "
             "encoder's launch each -- a step has the three training launches once per encoder, on two streams"]
    bench_kernels(a, dev, lines)
    lines += ["#", f"# 2. CREMA-D shapes, B = {a.batch}, bf16, concat head: a trainer on a model with the stacks against the same trainer class on "
              f"a model without, {a.rounds} rounds x ({a.warmup} warm-up + {a.steps} timed steps) per setting, alternating, the order swapped "
              "every round; ms per step"]
    for mode in ("joint", "multi-task"):
        bench_step(a, dev, lines, mode)
    if parent_lines:
        lines += ["#", f"# 3. bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup} --no-extra --no-comparator --no-f32 (the flagship DGL "
                  "step; the branch is not on it) on a checkout of the parent commit and on this commit, alternating in one job on the "
                  "same box, a process each, before section 1; ms per step"] + parent_lines
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
