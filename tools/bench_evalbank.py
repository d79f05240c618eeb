#!/usr/bin/env python3
"""The evaluation report's score bank (csrc/evalbank.hip) alone and inside valid(), on one MI355X.

    python tools/bench_evalbank.py [--rounds 7] [--launches 500] [--parent-tree DIR] [--out profiles/evalbank_bench.txt]

1. gdl_eval_bank_append (sets = 3) at B = 64 and n = 6 / 34 / 309 beside gdl_eval_count alone on the same logits: back-to-back
   launches between two device events, us per launch; median of the rounds, lowest and highest round in brackets.
2. gdl_eval_bank_ap (the AP kernel and the mAP kernel behind it) at n = 34, N = 2 560 (Kinetics-Sounds-like) and n = 309,
   N = 15 360 (VGGSound-like), sets = 3, random logits; for orientation scikit-learn's average_precision_score on one host core
   over the same stored probabilities, if it is installed.
3. One trainer's valid() over 16 batches (B = 64, CREMA-D shapes, bf16) without a bank, and with one including reset() and
   report(); report() alone; host clock.
4. With --parent-tree (a built checkout of the parent commit): `bench.py --gpus 1` (the flagship step, which never touches the
   bank) there and here, alternating, a fresh process each -- run BEFORE this process opens the device.
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
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup), "--no-extra",
           "--no-comparator", "--no-f32", "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k != "GDL_LIB"}
    p = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"bench_evalbank: bench.py in {tree} ended with {p.returncode}:\n{p.stderr[-2000:]}")
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
              f"# this - parent (means) = {d:+.4f} ms; spread between the runs of one tree = {sp:.4f} ms: the flagship step "
              f"{'DIFFERS BY MORE THAN' if abs(d) > sp else 'lies within'} the job's own spread"]


def timed(fn, a, launches=None):
    """us per call: `rounds` rounds of back-to-back calls between two device events -> (median, lowest, highest)"""
    import numpy as np
    import torch

    launches = launches or a.launches
    us = []
    for _ in range(a.rounds):
        for _ in range(max(2, launches // 10)):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) / launches * 1e3)
    return float(np.median(us)), min(us), max(us)


def fmt(t):
    return f"{t[0]:10.2f} us ({t[1]:.2f} .. {t[2]:.2f})"


def bench_append(a, dev, lines):
    import torch

    import gdl
    from gdl import _lib as L

    st, B = L.cur_stream(), 64
    for n in (6, 34, 309):
        g = torch.Generator().manual_seed(n)
        outs = [(3 * torch.randn(B, n, generator=g)).to(dev) for _ in range(3)]
        lab = torch.randint(0, n, (B,), generator=g).to(dev)
        cnt = torch.zeros((4, n), dtype=torch.int64, device=dev)
        bank = gdl.ScoreBank(n, 1024, 3, dev)

        def count():
            L.call("gdl_eval_count", outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), lab.data_ptr(), B, n,
                   cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr(), cnt[3].data_ptr(), st)

        def append():
            L.call("gdl_eval_bank_append", bank.buf.data_ptr(), bank.buf.numel(), n, bank.capacity, 3, outs[0].data_ptr(),
                   outs[1].data_ptr(), outs[2].data_ptr(), lab.data_ptr(), B, 0, st)

        def both():
            count()
            append()

        tc, ta, tb = timed(count, a), timed(append, a), timed(both, a)
        lines.append(f"B = 64, n = {n:3d}:  gdl_eval_count {fmt(tc)}   gdl_eval_bank_append {fmt(ta)}   both, back to back {fmt(tb)}")
        print(lines[-1], flush=True)


def bench_ap(a, dev, lines):
    import numpy as np
    import torch

    import gdl

    for n, N in ((34, 2560), (309, 15360)):
        g = torch.Generator().manual_seed(N)
        bank = gdl.ScoreBank(n, N, 3, dev)
        lab = torch.randint(0, n, (N,), generator=g)
        sets = [3 * torch.randn(N, n, generator=g) for _ in range(3)]
        for s in sets:  # scores that lean to the label, as a trained model's do
            s[torch.arange(N), lab] += 2.0
        sets, lab = [s.to(dev) for s in sets], lab.to(dev)
        for o in range(0, N, 64):
            bank.append(sets[0][o:o + 64], sets[1][o:o + 64], sets[2][o:o + 64], lab[o:o + 64])
        rep = bank.report()
        st = gdl._lib.cur_stream()

        def ap_call():
            gdl._lib.call("gdl_eval_bank_ap", bank.buf.data_ptr(), bank.buf.numel(), n, N, 3, N, st)

        t = timed(ap_call, a, launches=a.ap_launches)
        t0 = time.perf_counter()
        bank.report()
        host = (time.perf_counter() - t0) * 1e3
        lines.append(f"n = {n:3d}, N = {N:5d}, sets = 3:  gdl_eval_bank_ap {fmt(t)}   report() on the host clock {host:.3f} ms   "
                     f"mAP {' '.join(f'{v:.4f}' for v in rep['mAP'])}, top-1 {' '.join(f'{v:.4f}' for v in rep['topk'][1])}")
        print(lines[-1], flush=True)
        try:
            from sklearn.metrics import average_precision_score
        except ImportError:
            lines.append("    scikit-learn is not installed here: no host figure from this machine")
            continue
        labs, probs = bank.scores()
        t0 = time.perf_counter()
        ap = np.array([[average_precision_score(labs == c, probs[s, c]) if (labs == c).any() else np.nan for c in range(n)]
                       for s in range(3)])
        sk = time.perf_counter() - t0
        diff = float(np.nanmax(np.abs(ap - rep["ap"])))
        lines.append(f"    for orientation: scikit-learn's average_precision_score, {3 * n} calls on one host core over the same "
                     f"probabilities: {sk * 1e3:.1f} ms; largest |difference| to the device's ap {diff:.2e}")
        print(lines[-1], flush=True)


def bench_valid(a, dev, lines):
    import numpy as np
    import torch

    import bench
    import gdl
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    wl, B, nb = bench.WORKLOADS["cremad"], 64, 16
    setup_seed(0)
    model = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset=wl["dataset"], modality="full", batch_size=B))
    model.apply(weight_init)
    tr = DGLTrainer(model.to(dev).train(), lr=2e-3, max_norm=40.0, dtype="bf16", alpha=wl["alpha"])
    g = torch.Generator(device="cpu").manual_seed(1234)
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]
    tr.step(*data[0])
    batches = [data[i % 4] for i in range(nb)]
    bank = gdl.ScoreBank(wl["n_classes"], nb * B, 3, dev)
    plain, banked, rep_ms = [], [], []
    for r in range(a.rounds + 1):
        for with_bank in ((False, True) if r % 2 == 0 else (True, False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if with_bank:
                bank.reset()
                acc = tr.valid(batches, bank=bank)
                t1 = time.perf_counter()
                rep = bank.report()
                rep_ms.append((time.perf_counter() - t1) * 1e3)
            else:
                acc = tr.valid(batches)
            (banked if with_bank else plain).append((time.perf_counter() - t0) * 1e3)
    plain, banked, rep_ms = plain[1:], banked[1:], rep_ms[1:]  # (the first round warms up)
    assert rep["topk"][1][0] == acc[0]
    tr.close()
    for name, v in (("valid(batches)", plain), ("reset + valid(batches, bank) + report()", banked), ("  of which report()", rep_ms)):
        lines.append(f"{name:<42}{float(np.median(v)):9.3f} ms ({min(v):.3f} .. {max(v):.3f})")
        print(lines[-1], flush=True)
    d = float(np.median(banked)) - float(np.median(plain))
    lines.append(f"# with a bank - without = {d:+.3f} ms over {nb} batches = {d / nb * 1e3:+.1f} us per batch; spread of the plain "
                 f"valid() between rounds {max(plain) - min(plain):.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--ap-launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: bench.py there and here (section 4)")
    ap.add_argument("--pairs", type=int, default=3, help="bench.py runs per tree in section 4")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    parent_lines = []
    if a.parent_tree:  # fresh processes, before this one opens the device
        bench_parent(a, parent_lines)
    import torch

    from gdl import _lib as L

    if not torch.cuda.is_available():
        raise SystemExit("bench_evalbank: no GPU visible; a timing needs the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    lines = [f"bench_evalbank: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}; {a.rounds} rounds; a figure is the median "
             "of the rounds, in brackets the lowest and highest round",
             f"1. one launch per batch, sets = 3 (fused, audio, visual); {a.launches} back-to-back launches per round, device events"]
    bench_append(a, dev, lines)
    lines.append(f"2. the report's launch pair (AP kernel + mAP kernel); {a.ap_launches} back-to-back calls per round, device events")
    bench_ap(a, dev, lines)
    lines.append("3. DGLTrainer.valid() over 16 batches, B = 64, CREMA-D shapes, bf16, concat head; host clock, the one host copy inside")
    bench_valid(a, dev, lines)
    if parent_lines:
        lines += [f"4. bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup} --no-extra --no-comparator --no-f32 --no-cpu-baseline (the "
                  "flagship step) on a checkout of the parent commit and on this commit, alternating in one job, a process each, "
                  "before section 1; ms per step"] + parent_lines
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
