#!/usr/bin/env python3
"""bench.py -- CREMA-D DGL train step on N MI355X (one process per GPU, RCCL over xGMI).

    python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
    python bench.py --gpus N --steps K --warmup W        (starts the launcher below as a child process itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one full pass of the hot path of /root/reference/main_dgl.py:97-154 over one
synthetic CREMA-D-shaped batch that is already resident in HBM: both ResNet18 encoders forward,
the gradient-truncated fusion head + three cross-entropies, both encoder backwards, the
per-bucket gradient all-reduce (N > 1), global-norm clipping, the logged per-encoder gradient
statistics and the SGD(momentum, weight decay) update -- nothing skipped, nothing cached.
Rank 0 prints ONE JSON line (see the driver contract).  A plain run sets up, warms up, times the
K steps, writes the last step's outputs if --dump-outputs is given and prints that line; every other
figure below is measured only with --full.  `roofline` is measured live with HIP
events around every launch of the dominant kernel inside the timed region; `cpu_baseline` times the
PyTorch-CPU-operator restatement of the step (oracle/torch_step.py; the plain-C port of oracle/ rides
along as `c_port`) on this machine's host cores; `comparators.torch_rocm` times that same restatement
on the MI355X with stock PyTorch-ROCm operators (MIOpen, bf16 autocast, channels_last) -- a diagnostic,
not the product path; `extra_workloads` are short legs of the Kinetics-Sounds shapes (configs[2]) and of
the VGGSound shapes with the Swin-T visual branch (configs[4]) so that their numbers are driver-visible.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

# the workloads of BASELINE.json's configs: configs[1] (the metric's own, default) and configs[2] (Kinetics-Sounds shapes;
# 34 logits as the reference builds it, basic_model.py:17 -- BASELINE says 31, the cost difference is nil)
WORKLOADS = {
    "cremad": {"dataset": "CREMAD", "n_classes": 6, "spec": (257, 188), "alpha": 4.0, "gflop": 42.567,
               "name": "CREMA-D DGL (main_dgl.py, ConcatFusion_DGL) ResNet18 a+v, spec 1x257x188 + frames 3x3x224x224, "
                       "alpha=4, SGD lr 2e-3 mom .9 wd 1e-4, clip 40",
               "metric": "audio-visual samples/sec, CREMA-D DGL train step (whole job)"},
    "ks": {"dataset": "KineticSound", "n_classes": 34, "spec": (129, 626), "alpha": 2.0, "gflop": 50.563,
           "name": "Kinetics-Sounds DGL (main_dgl.py, ConcatFusion_DGL) ResNet18 a+v, spec 1x129x626 + frames 3x3x224x224, "
                   "34 logits, alpha=2, SGD lr 2e-3 mom .9 wd 1e-4, clip 40",
           "metric": "audio-visual samples/sec, Kinetics-Sounds DGL train step (whole job)"},
    # configs[4]'s data shapes (VGGSound: the Kinetics-Sounds shapes with 309 logits) on the ResNet18 visual branch (the
    # Swin-T branch of that configuration is the next entry)
    "vggsound": {"dataset": "VGGSound", "n_classes": 309, "spec": (129, 626), "alpha": 2.0, "gflop": 50.563,
                 "name": "VGGSound-shaped DGL (main_dgl.py, ConcatFusion_DGL) ResNet18 a+v, spec 1x129x626 + frames 3x3x224x224, "
                         "309 logits, alpha=2, SGD lr 2e-3 mom .9 wd 1e-4, clip 40",
                 "metric": "audio-visual samples/sec, VGGSound-shaped DGL train step (whole job)"},
    # configs[4] proper: the VGGSound shapes with the Swin-T visual branch (SURVEY row N4 -- a composition the reference's
    # main_dgl.py cannot build, models.basic_model.AVClassifier_DGL_Swin).  Arithmetic per sample: audio ResNet18 at
    # 129 x 626 13.66 GFLOP (the ks figure minus its 36.9 GFLOP visual ResNet) + 3 frames x 3 x 4.51 GFLOP of Swin-T
    "vggsound_swin": {"dataset": "VGGSound", "n_classes": 309, "spec": (129, 626), "alpha": 2.0, "gflop": 54.25, "swin": True,
                      "name": "VGGSound-shaped DGL, ResNet18 audio + Swin-T visual (embed 96, depths 2-2-6-2, heads 3-6-12-24, "
                              "window 7, drop_path 0) + ConcatFusion_DGL over 512+768, spec 1x129x626 + frames 3x3x224x224, 309 "
                              "logits, alpha=2, SGD lr 2e-3 mom .9 wd 1e-4, clip 40",
                      "metric": "audio-visual samples/sec, VGGSound-shaped DGL train step with a Swin-T visual branch (whole job)"},
}
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}  # MI355X_MICROARCH.md (dense)
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64, help="per-GPU batch (BASELINE config 2: 64)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--workload", default="cremad", choices=sorted(WORKLOADS),
                    help="cremad = BASELINE configs[1] (the metric's configuration); ks = configs[2] shapes; vggsound = configs[4]'s "
                         "data shapes on the ResNet18 pair; vggsound_swin = configs[4] (Swin-T visual branch)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=16, help="samples in the C-port CPU step (about 10-20 s of CPU work)")
    ap.add_argument("--cpu-torch-batch", type=int, default=8, help="samples in the PyTorch-operator CPU step (3 warm-up + 5 timed)")
    ap.add_argument("--no-f32", action="store_true", help="skip the short exact-f32 run behind the f32_exact field")
    ap.add_argument("--batches", type=int, default=8, help="distinct synthetic batches resident in HBM, fed round robin")
    ap.add_argument("--cpu-threads", type=int, default=0, help="0 = min(host cores, 64)")
    ap.add_argument("--no-prof", action="store_true", help="do not tap per-kernel HIP events in the timed region")
    ap.add_argument("--side-stream", choices=("auto", "on", "off"), default="auto",
                    help="the visual weight gradients' own stream: auto = on without a process group, off with one")
    ap.add_argument("--phases", action="store_true", help="also report forward / head / backward / optimizer phase times")
    ap.add_argument("--no-extra", action="store_true", help="skip the short ks / vggsound_swin legs behind extra_workloads")
    ap.add_argument("--drop-path", type=float, default=0.0,
                    help="vggsound_swin only: stochastic-depth rate of the Swin branch (the reference constructor's default is 0.1; "
                         "the committed line is quoted at 0)")
    ap.add_argument("--no-comparator", action="store_true", help="skip comparators.torch_rocm (stock PyTorch-ROCm step)")
    ap.add_argument("--comparator-find", action="store_true",
                    help="comparators.torch_rocm in MIOpen find mode, all variants (minutes of warm-up; profiles/ keeps one such run)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the per-kernel table and roofline tap, clip statistics, "
                         "f32_exact, extra_workloads, comparators, cpu_baseline and (N > 1) comm; the --no-* flags above thin it out")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned to its caller as DIR/<name>.npy (float32 / float64)")
    return ap.parse_args()


def src_hash():
    """sha256 over the kernel / engine sources the loaded library was built from: stamps PMC measurements."""
    import glob
    import hashlib

    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "iccv2025-gdl_amd", "csrc", "*.hip")) +
                    glob.glob(os.path.join(ROOT, "iccv2025-gdl_amd", "csrc", "*.h")) +
                    glob.glob(os.path.join(ROOT, "iccv2025-gdl_amd", "csrc", "*.cpp"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def cpu_baseline(batch, torch_batch, threads, wl):
    """The DGL step on this machine's host cores, on a bounded sample, two ways (both `kind: port` -- restatements of
    the reference's arithmetic, never its files): the PyTorch-operator restatement (oracle/torch_step.py: ATen / oneDNN
    kernels, what the reference itself runs on a CPU; B=8, 3 warm-up + 5 timed steps) is the
    reported baseline, the plain-C port (oracle/gdl_oracle.c, the parity oracle; 1 warm-up + 1 timed step) rides along."""
    from oracle import fixtures as fx
    from oracle import oracle as orc
    from oracle.torch_step import TorchStep

    cores = os.cpu_count() or 1
    thr = threads if threads > 0 else min(cores, 64)
    P, Bf = fx.model_state(wl["n_classes"], "concat_dgl")
    # ---- PyTorch operators
    torch.set_num_threads(thr)
    spec, image, label = fx.make_batch(0, torch_batch, wl["spec"], 3, (224, 224), wl["n_classes"])
    ts = TorchStep(P, Bf)
    for _ in range(3):
        ts.train_step(spec, image, label, wl["alpha"], 2e-3)
    t0 = time.time()
    for _ in range(5):
        ts.train_step(spec, image, label, wl["alpha"], 2e-3)
    dt_t = (time.time() - t0) / 5
    del ts
    # ---- C port
    orc.set_num_threads(thr)
    model = orc.AVModel(P, Bf, "dgl")
    spec, image, label = fx.make_batch(0, batch, wl["spec"], 3, (224, 224), wl["n_classes"])
    t0 = time.time()
    model.train_step(spec, image, label, wl["alpha"], 2e-3)
    t1 = time.time()
    model.train_step(spec, image, label, wl["alpha"], 2e-3)
    dt_c = time.time() - t1
    c_port = {"value": round(batch / dt_c, 3), "unit": "samples/s", "cores": thr, "kind": "port",
              "sample": f"oracle/ C port, {wl['dataset']} T=3 DGL step, B={batch}, fp32, 1 warm-up ({t1 - t0:.1f} s) + 1 timed "
                        f"step ({dt_c:.1f} s) on {thr} of {cores} host threads"}
    return {"value": round(torch_batch / dt_t, 3), "unit": "samples/s", "cores": thr, "kind": "port",
            "sample": f"oracle/torch_step.py (PyTorch {torch.__version__} CPU operators), {wl['dataset']} T=3 DGL step, "
                      f"B={torch_batch}, fp32, 3 warm-up + 5 timed steps ({dt_t:.2f} s each) on {thr} of {cores} host threads",
            "c_port": c_port}


def torch_rocm_comparator(wl, B, dev, find=False):
    """The SAME step with stock PyTorch-ROCm operators on this GPU (oracle/torch_step.py on `dev`: MIOpen convolutions /
    batch norm, rocBLAS head, fp32 master weights, foreach clip + hand-written SGD as in the restatement).  Diagnostic only
    -- with no published number for the metric this is the one figure that says what the reference's own arithmetic gets
    on an MI355X from the stock stack.  Variants: bf16 autocast + channels_last (the fastest form the stock stack has,
    reported as `value`), and with --comparator-find also bf16 / fp32 NCHW (fp32 NCHW is what main_dgl.py literally runs).
    `find`: MIOpen find mode (cudnn.benchmark = True: the library benchmarks every solver per shape, ~2-3 minutes of
    warm-up per variant on this pool) instead of its immediate-mode heuristics.  torch.backends.cudnn.deterministic is
    switched OFF for the measurement: the reference's setup_seed() (utils/utils.py:7-14) switches it on, which pins MIOpen
    to its slowest solvers (measured here: 595 ms / step fp32, 7.3 s / step bf16 channels_last) -- that figure is reported
    separately as `deterministic_as_reference` under --comparator-find."""
    from oracle import fixtures as fx
    from oracle.torch_step import TorchStep

    prev = (torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic)
    try:
        P, Bf = fx.model_state(wl["n_classes"], "concat_dgl")
        g = torch.Generator(device="cpu").manual_seed(4321)
        data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
                 torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]

        def run(ac, cl, det, nwarm, n):
            torch.backends.cudnn.benchmark = bool(find) and not det
            torch.backends.cudnn.deterministic = det
            ts = TorchStep(P, Bf, device=dev, autocast=ac, channels_last=cl)
            for i in range(nwarm):
                ts.train_step(*data[i % 4], wl["alpha"], 2e-3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                ts.train_step(*data[i % 4], wl["alpha"], 2e-3)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            del ts
            torch.cuda.empty_cache()
            return {"ms_per_step": round(dt * 1e3, 3), "value": round(B / dt, 2), "unit": "samples/s", "steps": n}

        out = {"bf16_channels_last": run(torch.bfloat16, True, False, 6, 20)}
        if find:
            out["bf16_nchw"] = run(torch.bfloat16, False, False, 6, 20)
            out["fp32_nchw"] = run(None, False, False, 6, 10)
            out["deterministic_as_reference"] = dict(run(None, False, True, 2, 3), note="fp32 NCHW with cudnn.deterministic = True, "
                                                     "as main_dgl.py -> setup_seed() leaves it")
        best = min(out.values(), key=lambda v: v["ms_per_step"] if "note" not in v else 1e30)
        return {"value": best["value"], "unit": "samples/s", "ms_per_step": best["ms_per_step"], "batch": B,
                "miopen_mode": "find (cudnn.benchmark)" if find else "immediate (heuristic solver choice)",
                "what": f"oracle/torch_step.py on the GPU: PyTorch {torch.__version__} eager operators (MIOpen / rocBLAS), bf16 autocast "
                        "+ channels_last, fp32 master weights, cudnn.deterministic off, 6 warm-up + 20 timed steps; diagnostic "
                        "comparator, not the product path", "variants": out}
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = prev


def build_model(wl, batch, dev):
    """The model exactly as main_dgl.py:230-246 builds it (random init; identical on every rank via the seed)."""
    from models.basic_model import AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    setup_seed(0)
    args = argparse.Namespace(fusion_method="concat", dataset=wl["dataset"], modality="full", batch_size=batch, pe=0)
    if wl.get("swin"):
        from models.basic_model import AVClassifier_DGL_Swin

        kw = dict(AVClassifier_DGL_Swin.SWIN_T, drop_path_rate=float(wl.get("drop_path", 0.0)))
        model = AVClassifier_DGL_Swin(args, swin_kwargs=kw)  # (the Swin branch keeps its own initialisation, swin_transformer.py:568-576:
        model.audio_net.apply(weight_init)   #  utils.weight_init would trip over PatchMerging's bias-free Linear)
        model.fusion_module.apply(weight_init)
    else:
        model = AVClassifier_DGL(args)
        model.apply(weight_init)
    model.to(dev)
    model.train()
    return model, args


DUMP_SAMPLE = 1 << 21  # elements kept of each flat arena by --dump-outputs (3 x 8 MB; the arenas hold 22 M+ each)


def dump_outputs(tr, res, out_dir):
    """What the last step handed its caller, as DIR/<name>.npy: the three logit sets, the losses and gradient statistics of
    DGLTrainer.read(), the BatchNorm running statistics, and a fixed seeded sample (same positions in every run of the same
    model) of the updated parameters, their gradients and the momentum."""
    os.makedirs(out_dir, exist_ok=True)
    n = tr.params.numel()
    idx = np.sort(np.random.default_rng(0).choice(n, size=min(n, DUMP_SAMPLE), replace=False))
    idx = torch.from_numpy(idx).to(tr.params.device)
    m = tr.model
    bn = [b.reshape(-1) for net in (m.audio_net, m.visual_net) for name, b in net.named_buffers()
          if name.endswith(("running_mean", "running_var"))]
    arrays = {"out": res["out"], "out_a": res["out_a"], "out_v": res["out_v"],
              "losses": [res["loss_f"], res["loss_a"], res["loss_v"]],
              "grad_stats": [res["total_norm"], res["clip_coef"], res["audio_grad_sum"], res["visual_grad_sum"]],
              "grad_norm": list(res["grad_norm"].values()), "grad_absmean": list(res["grad_absmean"].values()),
              "bn_running_stats": torch.cat(bn).float().cpu().numpy() if bn else [],
              "params_sample": tr.params[idx].cpu().numpy(), "grads_sample": tr.grads[idx].cpu().numpy(),
              "momentum_sample": tr.momentum[idx].cpu().numpy()}
    for name, v in arrays.items():
        v = np.asarray(v)
        np.save(os.path.join(out_dir, name + ".npy"), v if v.dtype in (np.float32, np.float64) else v.astype(np.float64))


def extra_leg(name, a, dev, lib, collect, steps=30, warmup=15):
    """A short driver-visible leg of another BASELINE configuration (N = 1): its own ms_per_step and the in-step roofline
    of its dominant kernel.  Same step, same trainer, same taps as the main measurement.  15 + 2 warm-up and 30 timed steps
    (round 3's 5 + 2 / 10 read 15 % above the 100-step runs: clocks and the allocator had not settled)."""
    from gdl.trainer import DGLTrainer

    wl = WORKLOADS[name]
    model, _ = build_model(wl, a.batch, dev)
    tr = DGLTrainer(model, lr=2e-3, alpha=wl["alpha"], momentum=0.9, weight_decay=1e-4, max_norm=40.0, dtype=a.dtype)
    g = torch.Generator(device="cpu").manual_seed(99)
    B = a.batch
    data = [(torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
             torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)) for _ in range(4)]
    for i in range(warmup):
        tr.step(*data[i % 4])
    torch.cuda.synchronize()
    lib.gdl_prof_set_filter(None)
    lib.gdl_prof_enable(1)
    for i in range(2):
        tr.step(*data[i % 4])
    torch.cuda.synchronize()
    lib.gdl_prof_enable(0)
    table = collect(2)
    dom = table[0]["kernel"]
    lib.gdl_prof_set_filter(dom.encode())
    torch.cuda.synchronize()
    tapped = 0
    t0 = time.perf_counter()
    for i in range(steps):  # (the tap samples every 4th step of these shorter runs)
        lib.gdl_prof_enable(1 if i % 4 == 0 else 0)
        tapped += i % 4 == 0
        tr.step(*data[i % 4])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    lib.gdl_prof_enable(0)
    d = [k for k in collect(max(1, tapped)) if k["kernel"] == dom][0]
    lib.gdl_prof_set_filter(None)
    res = tr.read()
    top = [{"kernel": k["kernel"], "ms_per_step": k["ms_per_step"], "frac": k["frac"], "bound": k["bound"]} for k in table[:6]]
    del tr, model
    torch.cuda.empty_cache()
    return {"workload": wl["name"], "metric": wl["metric"], "value": round(B / dt, 2), "unit": "samples/s",
            "ms_per_step": round(dt * 1e3, 3), "steps": steps, "warmup": warmup + 2, "dtype": a.dtype, "batch": B,
            "step_tflops": round(B / dt * wl["gflop"] / 1e3, 2),
            "mfma_frac_end_to_end": round(B / dt * wl["gflop"] / 1e3 / MFMA_PEAK_TFLOPS[a.dtype], 4),
            "loss_f": round(res["loss_f"], 5), "total_norm": round(res["total_norm"], 4),
            "roofline": {"bound": d["bound"], "kernel": d["kernel"], "achieved": d["achieved"], "unit": d["unit"],
                         "peak": MFMA_PEAK_TFLOPS[a.dtype] if d["bound"] == "mfma" else HBM_PEAK_GBS, "frac": d["frac"],
                         "avg_launch_us": d["avg_us"], "launches_per_step": d["launches_per_step"]},
            "top_kernels": top}


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...
    bench.py <the same arguments>` as a CHILD process (one rank per GPU over RCCL, the form the driver contract names), pass
    its output through -- rank 0's single JSON line included -- and return its exit code.  The parent never initialises the
    device (no exec of a process that has: the child is a fresh interpreter), so this is safe on the GPU pool."""
    import socket
    import subprocess

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL's cross-process buffers on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"bench.py: --gpus {n} without WORLD_SIZE: launching {' '.join(cmd[1:9])} ...", file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env, cwd=os.getcwd())


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world and world > 1:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # typed plainly (`python bench.py --gpus N`): launch the N ranks ourselves.  Nothing above this line has touched the GPU
        sys.exit(self_launch(a.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py: no MI355X visible; the HIP path has no CPU fallback")
    # test plumbing (tests/test_ddp_gpu.py): GDL_BENCH_BACKEND=gloo with GDL_BENCH_ONE_DEVICE=1 runs the N-rank
    # control flow on a box with a single GPU (RCCL refuses two ranks on one device); never used for numbers
    backend = os.environ.get("GDL_BENCH_BACKEND", "nccl")
    if os.environ.get("GDL_BENCH_ONE_DEVICE") == "1":
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    pg = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)  # RCCL
        else:
            dist.init_process_group(backend)
        pg = dist.group.WORLD
    elif os.environ.get("GDL_BENCH_FORCE_PG") == "1":
        # test plumbing: the data-parallel code path (bucketed RCCL all-reduce, its stream) with a one-rank group on one GPU
        import torch.distributed as dist

        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29533", rank=0, world_size=1, device_id=dev)
        pg = dist.group.WORLD

    from gdl import _lib as L
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier_DGL
    from utils.utils import setup_seed, weight_init

    lib = L.load()
    wl = WORKLOADS[a.workload]
    if wl.get("swin") and a.drop_path > 0:  # (a different workload from the committed one: said in its name)
        wl = dict(wl, drop_path=a.drop_path, name=wl["name"].replace("drop_path 0)", f"drop_path {a.drop_path:g})"))
    model, args = build_model(wl, a.batch, dev)
    if wl.get("swin"):
        a.no_f32 = a.no_cpu_baseline = a.no_comparator = True  # (those legs are written for the ResNet18 pair)
    tr = DGLTrainer(model, lr=2e-3, alpha=wl["alpha"], momentum=0.9, weight_decay=1e-4, max_norm=40.0, dtype=a.dtype,
                    process_group=pg, visual_side_stream={"auto": None, "on": True, "off": False}[a.side_stream])
    # synthetic CREMA-D batch, seed 1234 + rank, resident on the device
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)
    B = a.batch
    # `--batches` distinct batches (resident in HBM, fed round robin): a single repeated batch is memorised within a
    # few dozen steps, after which the losses vanish and the clip is never active
    data = []
    for _ in range(max(1, a.batches)):
        data.append((torch.randn(B, *wl["spec"], generator=g).to(dev), torch.randn(B, 3, 3, 224, 224, generator=g).to(dev),
                     torch.randint(0, wl["n_classes"], (B,), generator=g).to(dev)))
    counter = [0]
    # (total norm, clip coefficient) of every step of the timed region, copied device-to-device behind each step (8 bytes on
    # the step's own stream: a measuring tap like the HIP events, read once after the region) -> clip_active_steps
    if a.full:
        tr.stats_log = torch.zeros((a.steps, 2), device=dev)

    def step():
        spec, image, label = data[counter[0] % len(data)]
        counter[0] += 1
        tr.step(spec, image, label)

    def barrier():
        if world > 1:
            import torch.distributed as dist

            dist.barrier(device_ids=[local]) if backend == "nccl" else dist.barrier()

    import ctypes

    def collect(nsteps):
        """Fold the tap's records into a per-kernel table (sorted by device time per step)."""
        ns = lib.gdl_prof_nslots()
        n_l = (ctypes.c_int64 * max(ns, 1))()
        n_ms = (ctypes.c_double * max(ns, 1))()
        n_w = (ctypes.c_double * max(ns, 1))()
        L.call("gdl_prof_collect", n_l, n_ms, n_w)
        n_fl = (ctypes.c_double * max(ns, 1))()
        n_by = (ctypes.c_double * max(ns, 1))()
        L.call("gdl_prof_collect_floor", n_fl, n_by)
        table = []
        for s in range(ns):
            if n_l[s] == 0:
                continue
            bound = "mfma" if lib.gdl_prof_slot_bound(s) == 1 else "hbm"
            rate = n_w[s] / (n_ms[s] * 1e-3)  # flop/s or byte/s
            peak = MFMA_PEAK_TFLOPS[a.dtype] if bound == "mfma" else HBM_PEAK_GBS
            ach = rate / 1e12 if bound == "mfma" else rate / 1e9
            row = {"kernel": lib.gdl_prof_slot_name(s).decode(), "bound": bound,
                   "launches_per_step": n_l[s] / nsteps, "avg_us": round(n_ms[s] / n_l[s] * 1e3, 2),
                   "ms_per_step": round(n_ms[s] / nsteps, 4), "achieved": round(ach, 2),
                   "unit": "TFLOP/s" if bound == "mfma" else "GB/s", "frac": round(ach / peak, 4),
                   # what `frac` is a fraction of: the MFMA peak (flops) or the HBM peak (bytes)
                   "frac_of": bound}
            if bound == "mfma" and n_by[s] > 0:
                # combined roofline: every launch priced against the roof that binds IT, max(flop / MFMA peak, algorithmic
                # bytes / HBM peak) -- the layer-1 launches of the convolutions sit at the HBM ridge
                row["frac_combined"] = round(n_fl[s] / n_ms[s], 4)
                row["algorithmic_mbytes_per_launch"] = round(n_by[s] / n_l[s] / 1e6, 2)
            table.append(row)
        table.sort(key=lambda k: -k["ms_per_step"])
        return table

    L.call("gdl_prof_set_peaks", MFMA_PEAK_TFLOPS[a.dtype] * 1e12, HBM_PEAK_GBS * 1e9)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    prof = a.full and not a.no_prof and rank == 0
    kernels, dominant = None, None
    if a.full and not a.no_prof:
        # untimed calibration: every launch tapped (costs ~10 % throughput), gives the per-kernel table and
        # names the dominant kernel; the timed region then taps ONLY that kernel's launches.  Every rank runs
        # the three steps (they contain the gradient all-reduces); only rank 0 taps.
        if prof:
            lib.gdl_prof_set_filter(None)
            lib.gdl_prof_enable(1)
        for _ in range(3):
            step()
        if prof:
            lib.gdl_prof_enable(0)
            kernels = collect(3)
            dominant = kernels[0]["kernel"]
            lib.gdl_prof_set_filter(dominant.encode())
    barrier()
    # The dominant kernel's launches carry HIP event pairs (hipExtLaunchKernelGGL) -- and an event-stamped launch does not pipeline
    # with its neighbours on the stream the way a plain one does: tapping all 26 launches of every step costs the timed region
    # ~1.5 % (5.62 vs 5.54 ms on one box).  The tap therefore samples every TAP_EVERY-th step of the timed region (first step
    # included): the roofline figures are averages over those steps' launches, the other steps run as the job does.
    TAP_EVERY = 10  # (260 tapped launches in the default 100-step run; every 4th step until round 5 cost 0.4 % of the timed region)
    tapped = 0
    torch.cuda.synchronize()
    tr.stats_log_pos = 0
    t0 = time.perf_counter()
    for i in range(a.steps):
        if prof:
            on = i % TAP_EVERY == 0
            lib.gdl_prof_enable(1 if on else 0)
            tapped += on
        step()
    torch.cuda.synchronize()
    barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    tr.stats_log_pos = None
    clip_log = tr.stats_log.cpu().numpy() if tr.stats_log is not None else None
    if world > 1:
        import torch.distributed as dist

        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    res = tr.read()
    if a.dump_outputs and rank == 0:  # (before anything below runs more steps or overwrites the arenas)
        dump_outputs(tr, res, a.dump_outputs)
    roof = None
    if prof:
        lib.gdl_prof_enable(0)
        d = [k for k in collect(max(1, tapped)) if k["kernel"] == dominant][0]
        lib.gdl_prof_set_filter(None)
        # HBM bytes per launch from the PMC counters: they need their own rocprofv3 --pmc passes (tools/pmc_kernels.sh
        # over this very command), so the committed measurement is read back -- but only if it was taken on the kernel
        # sources this library was built from (hash stamp), for this workload / dtype / batch; otherwise null
        traffic = None
        try:
            import glob

            # (the newest committed PMC table: profiles/rNN_pmc_kernels.json, tools/pmc_kernels.sh)
            pm = json.load(open(sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_kernels.json")))[-1]))
            # the tap names a kernel without its template arguments: launch-weighted mean over its instantiations
            ks = [v for n, v in pm.get("kernels", {}).items() if n == d["kernel"] or n.startswith(d["kernel"] + "<")]
            if (ks and pm.get("src_hash") == src_hash() and pm.get("dtype") == a.dtype and pm.get("batch") == B and
                    pm.get("workload") == a.workload):
                nl = sum(v["launches_per_step"] for v in ks)
                traffic = round(sum(v["hbm_bytes_per_launch"] * v["launches_per_step"] for v in ks) / nl)
        except (OSError, ValueError, KeyError, IndexError):
            pass
        roof = {"bound": d["bound"], "achieved": d["achieved"], "peak": MFMA_PEAK_TFLOPS[a.dtype] if d["bound"] == "mfma"
                else HBM_PEAK_GBS, "unit": d["unit"], "frac": d["frac"], "traffic": traffic, "kernel": d["kernel"],
                "avg_launch_us": d["avg_us"], "launches_per_step": d["launches_per_step"], "frac_of": d["frac_of"],
                "tapped_steps": tapped, "tapped_steps_note": f"every {TAP_EVERY}th step of the timed region carries the event pairs"}
        if "frac_combined" in d:
            roof["combined"] = {"frac": d["frac_combined"], "algorithmic_mbytes_per_launch": d["algorithmic_mbytes_per_launch"],
                                "note": "sum over the launches of max(flop / MFMA peak, algorithmic bytes / HBM peak) / measured time"}
    if prof and world == 1 and kernels and not wl.get("swin"):
        # The same kernels WITHOUT contention: each encoder's forward + backward on its own, weight gradients on the
        # chain's stream -- every launch has the device to itself.  The step's table says what a launch costs beside the
        # other streams (what the job pays); this one says what the kernel itself does (`roofline.alone`).
        # (a measurement after the timed region: it advances the BatchNorm running statistics and overwrites the gradient
        # arena; everything reported from the training run -- losses, norms, clip_log -- has been read above)
        had_side = tr.eng_v.lane() == "owned"
        tr.eng_v.side_stream(False)
        tr.eng_a.borrow_side_stream(None)  # (DGLTrainer.step binds the caller's stream again by itself)
        spec, image, _ = data[0]
        nf = tr.nf
        lib.gdl_prof_set_filter(None)
        lib.gdl_prof_enable(1)
        for eng, x, gv, df, feat in ((tr.eng_v, image, tr.gviews[nf + 60:nf + 120], tr.dfv, tr.fv),
                                     (tr.eng_a, spec.unsqueeze(1), tr.gviews[nf:nf + 60], tr.dfa, tr.fa)):
            for _ in range(3):
                eng.forward(x, True, feat_out=feat)
                eng.backward(gv, dfeat=df)
        torch.cuda.synchronize()
        lib.gdl_prof_enable(0)
        alone = {k["kernel"]: k for k in collect(3)}
        tr.eng_v.side_stream(had_side)  # exactly the configuration the timed region ran in
        for k in kernels:
            if k["kernel"] in alone:
                k["alone_avg_us"], k["alone_frac"] = alone[k["kernel"]]["avg_us"], alone[k["kernel"]]["frac"]
                if "frac_combined" in alone[k["kernel"]]:
                    k["alone_frac_combined"] = alone[k["kernel"]]["frac_combined"]
        if roof and roof["kernel"] in alone:
            al = alone[roof["kernel"]]
            roof["alone"] = {"avg_launch_us": al["avg_us"], "achieved": al["achieved"], "frac": al["frac"],
                             "frac_combined": al.get("frac_combined"),
                             "note": "same launches with nothing else on the device (encoders run one after the other, "
                                     "no side stream)"}
    phases = None
    if a.phases:  # (every rank runs the extra steps: they contain collectives)
        tr.phase_events = []
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        ev = tr.phase_events
        tr.phase_events = None
        acc = {}
        starts = [i for i, (n, _) in enumerate(ev) if n == "start"] + [len(ev)]
        for lo, hi in zip(starts[:-1], starts[1:]):  # one group of marks per step, whatever marks the step's form records
            for (n0, e0), (n1, e1) in zip(ev[lo:hi - 1], ev[lo + 1:hi]):
                acc.setdefault(n0 + "->" + n1, []).append(e0.elapsed_time(e1))
        phases = {k: round(sum(v) / len(v), 3) for k, v in acc.items()}
    comm = None
    if a.full and world > 1:
        # What the collectives cost and how much of it the backward hides: each bucket's all-reduce alone, and the
        # step with the reducer moving no data (same kernels, same events; NOT a valid training step -- timing only).
        import torch.distributed as dist

        buckets_ms = tr.reducer.time_buckets(torch.cuda.synchronize, barrier)
        tr.reducer.enabled = False
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        nn_ = max(10, a.steps // 4)
        for _ in range(nn_):
            step()
        torch.cuda.synchronize()
        barrier()
        t_nc = (time.perf_counter() - t0) / nn_ * 1e3
        tr.reducer.enabled = True
        t = torch.tensor([t_nc], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        t_nc = float(t.item())
        tot = sum(buckets_ms.values())
        exposed = max(0.0, elapsed / a.steps * 1e3 - t_nc)
        sent0, calls0 = tr.reducer.bytes_sent, tr.reducer.calls
        step()
        torch.cuda.synchronize()
        barrier()
        comm = {**tr.reducer.describe(),
                # what ONE step hands to all-reduce calls (five buckets = the whole 22.4 M-parameter gradient arena once)
                "allreduce_bytes_per_step": tr.reducer.bytes_sent - sent0, "allreduce_calls_per_step": tr.reducer.calls - calls0,
                "allreduce_alone_ms": buckets_ms, "allreduce_alone_sum_ms": round(tot, 4), "step_ms_without_comm": round(t_nc, 3),
                "exposed_ms": round(exposed, 3), "overlapped_frac": round(1.0 - min(1.0, exposed / tot), 4) if tot > 0 else None,
                "bucket_mbytes": {k: round((hi - lo) * 4 / 1e6, 3) for k, (lo, hi) in tr.bucket.items()}}
        # The two schedule choices that a one-GPU lease cannot decide, measured here on first contact with
        # real RCCL traffic: the visual weight gradients' side stream (a fifth stream beside the collective's) and the
        # early-backward form (another collective order).  Every rank runs every variant (they contain collectives); the
        # headline `value` above is the default configuration's.
        if not wl.get("swin"):
            def timed(nsteps):
                for _ in range(3):
                    step()
                torch.cuda.synchronize()
                barrier()
                t0_ = time.perf_counter()
                for _ in range(nsteps):
                    step()
                torch.cuda.synchronize()
                barrier()
                t_ = torch.tensor([(time.perf_counter() - t0_) / nsteps * 1e3], device=dev, dtype=torch.float64)
                dist.all_reduce(t_, op=dist.ReduceOp.MAX)
                return round(float(t_.item()), 3)

            vis0 = "caller" if tr.visual_on_caller else ("owned" if tr.eng_v.lane() == "owned" else "off")
            early0, lane0 = tr.early_backward, tr.audio_on_caller
            variants = {}
            for vis in ("off", "owned", "caller"):  # where the visual engine's weight gradients run
                for early in (False, True):
                    for lane in (False, True):  # the audio engine's weight gradients on the caller's stream
                        if vis == "caller" and lane:
                            continue  # (one borrowed lane)
                        tr.visual_on_caller = vis == "caller"
                        tr.eng_v.side_stream(vis == "owned")
                        tr.early_backward = early
                        tr.audio_on_caller = lane
                        variants[f"visual_wgrad_{vis}__early_backward_{'on' if early else 'off'}"
                                 f"__audio_lane_{'on' if lane else 'off'}"] = timed(nn_)
            tr.visual_on_caller = vis0 == "caller"
            tr.eng_v.side_stream(vis0 == "owned")
            tr.early_backward, tr.audio_on_caller = early0, lane0
            comm["schedule_variants_ms"] = variants
            comm["default_schedule"] = (f"visual_wgrad_{vis0}__early_backward_{'on' if early0 is not False else 'off'}"
                                        f"__audio_lane_{'on' if lane0 else 'off'}")
    if a.full and rank == 0:
        # the headline measurement is complete here: leave it on stderr (and in gpurun_out/ when that exists) BEFORE the secondary
        # legs below -- a hard fault in one of them (graph capture, MIOpen, an OOM kill) must not take it along
        head = {"metric": wl["metric"], "value": round(world * B * a.steps / elapsed, 2), "unit": "samples/s", "n_gpus": world,
                "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 3), "dtype": a.dtype,
                "roofline": roof, "provisional": "headline only; the full line follows on stdout"}
        sys.stderr.write("bench.py headline: " + json.dumps(head) + "\n")
        sys.stderr.flush()
        try:
            if os.path.isdir(os.path.join(ROOT, "gpurun_out")):
                with open(os.path.join(ROOT, "gpurun_out", "bench_headline.json"), "w") as f:
                    f.write(json.dumps(head) + "\n")
        except OSError:
            pass
    f32_exact = None
    if a.full and a.dtype == "bf16" and not a.no_f32:
        # the exact-parity mode (f32 storage, f32-input MFMA == an fmaf chain) on the same workload: a short run
        del tr
        torch.cuda.empty_cache()
        setup_seed(0)
        model32 = AVClassifier_DGL(args)
        model32.apply(weight_init)
        model32.to(dev)
        model32.train()
        tr32 = DGLTrainer(model32, lr=2e-3, alpha=wl["alpha"], momentum=0.9, weight_decay=1e-4, max_norm=40.0, dtype="f32",
                          process_group=pg)
        for i in range(3):
            tr32.step(*data[i % len(data)])
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        n32 = 10
        for i in range(n32):
            tr32.step(*data[i % len(data)])
        torch.cuda.synchronize()
        barrier()
        dt32 = time.perf_counter() - t0
        f32_exact = {"value": round(world * B * n32 / dt32, 2), "unit": "samples/s", "ms_per_step": round(dt32 / n32 * 1e3, 3),
                     "steps": n32, "note": "f32 storage + f32-input MFMA (bit-for-bit an fp32 fmaf chain): the parity mode, "
                                           "not the benchmark configuration"}
        del tr32
    extra = None
    comparators = None
    if a.full and world == 1 and pg is None:
        try:
            del tr
        except NameError:
            pass
        torch.cuda.empty_cache()
        if a.workload == "cremad" and not a.no_extra and not a.no_prof:
            extra = {}
            for name in ("ks", "vggsound_swin"):
                try:
                    extra[name] = extra_leg(name, a, dev, lib, collect)
                except Exception as e:  # a secondary leg must never take the headline line down
                    extra[name] = {"error": f"{type(e).__name__}: {e}"}
                    lib.gdl_prof_enable(0)
                    lib.gdl_prof_set_filter(None)
        if not a.no_comparator and a.dtype == "bf16":
            try:
                comparators = {"torch_rocm": torch_rocm_comparator(wl, B, dev, find=a.comparator_find)}
            except Exception as e:
                comparators = {"torch_rocm": {"error": f"{type(e).__name__}: {e}"}}
    if kernels:
        for k in kernels:
            if k["kernel"] == "gdl::sgd_kernel":
                k["bytes_note"] = ("20 n bytes charged: p, g, m read, p, m written; the 4 n-byte write-back of the clipped gradient "
                                   "happens only in steps whose clip is active (config.clip_regime)")
    if world > 1:
        import torch.distributed as dist

        barrier()
        dist.destroy_process_group()
    if rank != 0:
        return
    value = world * B * a.steps / elapsed
    clip = None if clip_log is None else (int((clip_log[:, 1] < 1.0).sum()), [round(float(clip_log[:, 0].min()), 4),
                                                                                round(float(clip_log[:, 0].max()), 4)])
    out = {
        "metric": wl["metric"],
        "value": round(value, 2), "unit": "samples/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(elapsed / a.steps * 1e3, 3), "timed_region_s": round(elapsed, 4),
        "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
        "config": {"workload": wl["name"],
                   "per_gpu_batch": B, "global_batch": B * world, "parallelism": f"dp{world}",
                   # which regime of clip_grad_norm_(40) the timed steps ran in (the kernels are the same; an inactive clip
                   # skips the 4 n-byte write-back of the scaled gradients in sgd_kernel)
                   "clip_regime": f"clip active in {clip[0]} of {a.steps} timed steps "
                                  f"({len(data)} distinct batches cycled, {a.warmup} warm-up steps)" if clip else None,
                   "buckets": "fusion head | audio layer4 | audio rest | visual layer4 | visual rest, RCCL all-reduce, layer4 "
                              "buckets overlapped with the rest of the backward" if world > 1 else "none"},
        "samples_per_sec_per_gpu": round(value / world, 2),
        "step_tflops": round(value * wl["gflop"] / 1e3, 2),
        "mfma_frac_end_to_end": round(value / world * wl["gflop"] / 1e3 / MFMA_PEAK_TFLOPS[a.dtype], 4),
        "loss_f": round(res["loss_f"], 5), "loss_a": round(res["loss_a"], 5), "loss_v": round(res["loss_v"], 5),
        "total_norm": round(res["total_norm"], 4),
        "clip_coef": round(res["clip_coef"], 4),
        # steps of the timed region in which clip_grad_norm_ actually scaled the gradients (coefficient < 1; the kernels do
        # the same work either way) and the range the global norm moved in
        "clip_active_steps": clip[0] if clip else None, "total_norm_range": clip[1] if clip else None,
        "roofline": roof, "kernels": kernels, "phases_ms": phases, "f32_exact": f32_exact, "comm": comm,
        "batches": len(data), "src_hash": src_hash(), "extra_workloads": extra, "comparators": comparators,
    }
    if a.full and world == 1 and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(a.cpu_batch, a.cpu_torch_batch, a.cpu_threads, wl)
    else:
        out["cpu_baseline"] = None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
