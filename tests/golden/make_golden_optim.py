#!/usr/bin/env python3
"""Generate the golden vectors of the `--optimizer Adam` / `--optimizer AdaGrad` steps by importing the reference
(PyTorch CPU fp32), as make_golden.py does for SGD.

Run once where the reference is available:  python tests/golden/make_golden_optim.py
The GPU tests read only the .npz outputs.

The step body is make_golden.run_step_case's restatement of main_dgl.py:97-154; the optimizer is built exactly as
main_dgl.py:252-256 builds it -- `optim.Adagrad(model.parameters(), lr=lr)` and
`optim.AdamW(model.parameters(), lr=lr, betas=(0.9, 0.999))`, every other argument torch's default.  Three steps per
fixture, so the Adam bias corrections of t = 1, 2 and 3 are all exercised.  Per step: the logged quantities, the
per-tensor parameter sums after optimizer.step(), the per-tensor sums of the optimizer state and the BatchNorm buffers
(no per-element gradients: the files stay small).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the repository root on sys.path)
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from oracle import fixtures as fx  # noqa: E402

STATE_KEYS = {"Adam": ("exp_avg", "exp_avg_sq"), "AdaGrad": ("sum",)}


def build_optimizer(kind, params, lr):
    """main_dgl.py:252-256, verbatim in what it passes."""
    if kind == "AdaGrad":
        return torch.optim.Adagrad(params, lr=lr)
    if kind == "Adam":
        return torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.999))
    raise ValueError(kind)


def optimizer_config(opt):
    """The hyperparameters the optimizer actually holds (its one parameter group)."""
    g = opt.param_groups[0]
    keys = ("lr", "betas", "eps", "weight_decay", "amsgrad", "lr_decay", "initial_accumulator_value", "maximize")
    return {k: (list(g[k]) if isinstance(g[k], tuple) else g[k]) for k in keys if k in g}


def run_optim_case(name, bm, bb, fm, kind, dataset, spec_hw, frames, image_hw, batch, alpha, steps, seed=0, lr=2e-3,
                   fusion="concat", swin_cfg=None, dtype=torch.float32, out_dir=HERE):
    torch.manual_seed(0)
    torch.set_num_threads(8)
    n_classes = fx.N_CLASSES[dataset]
    if swin_cfg is not None:
        model = mg._SwinDGL(bb, fm, n_classes, swin_cfg)
        ps, bs = fx.swin_dgl_state(n_classes, swin_cfg)
        assert [n for n, _ in model.named_parameters()] == list(ps)
        res = model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in {**ps, **bs}.items()}, strict=False)
        assert not res.unexpected_keys and all("relative_position_index" in k or "attn_mask" in k for k in res.missing_keys)
    else:
        args = argparse.Namespace(fusion_method=fusion, dataset=dataset, modality="full", batch_size=batch)
        model = bm.AVClassifier_DGL(args)
        mg._load(model, n_classes, fusion + "_dgl")
    model.to(dtype)  # (float64: the spread of two correct runs, tools/optim_golden_spread.py; float32 is the golden)
    named = [("module." + n, p) for n, p in model.named_parameters()]  # (DataParallel's prefix, main_dgl.py:244)
    opt = build_optimizer(kind, model.parameters(), lr)
    crit = nn.CrossEntropyLoss()
    out_d = {}
    cfg = dict(name=name, dataset=dataset, n_classes=n_classes, spec_hw=list(spec_hw), frames=frames, image_hw=list(image_hw),
               batch=batch, alpha=alpha, steps=steps, mode="dgl", seed=seed, lr=lr, max_norm=40.0, torch=torch.__version__,
               fusion=fusion, optimizer=kind, optimizer_torch=type(opt).__name__, optimizer_args=optimizer_config(opt))
    if swin_cfg is not None:
        cfg["swin"] = dict(swin_cfg)
    if dtype != torch.float32:
        cfg["dtype"] = str(dtype)
    out_d["config"] = np.array(json.dumps(cfg))
    model.train()
    for st in range(steps):
        spec, image, label = fx.make_batch(seed + st, batch, spec_hw, frames, image_hw, n_classes)
        spec, image, label = torch.from_numpy(spec), torch.from_numpy(image), torch.from_numpy(label)
        opt.zero_grad()  # main_dgl.py:97
        pre = f"s{st}."
        out, out_a, out_v = model(spec.unsqueeze(1).to(dtype), image.to(dtype))  # :100 (.float())
        loss_v = crit(out_v, label)
        loss_a = crit(out_a, label)
        loss_f = crit(out, label)
        ((loss_a + loss_v) * alpha).backward(retain_graph=True)  # :108-110
        for n, p in named:  # :114-119
            if "fusion" in str(n).split(".")[1]:
                p.grad = None
        loss_f.backward()  # :122
        out_d[pre + "out"] = out.detach().numpy()
        out_d[pre + "out_a"] = out_a.detach().numpy()
        out_d[pre + "out_v"] = out_v.detach().numpy()
        out_d[pre + "loss_f"] = np.float64(loss_f.item())
        out_d[pre + "loss_a"] = np.float64(loss_a.item())
        out_d[pre + "loss_v"] = np.float64(loss_v.item())
        total = nn.utils.clip_grad_norm_(model.parameters(), max_norm=40, norm_type=2)  # :129
        out_d[pre + "total_norm"] = np.float64(total.item())
        out_d[pre + "audio_grad_sum"] = np.float64(sum(torch.abs(p.grad).mean().item() for p in model.audio_net.parameters()))
        out_d[pre + "visual_grad_sum"] = np.float64(sum(torch.abs(p.grad).mean().item() for p in model.visual_net.parameters()))
        names, gn, isnone = [], [], []
        for n, p in model.named_parameters():
            names.append(n)
            isnone.append(int(p.grad is None))
            gn.append(0.0 if p.grad is None else float(p.grad.detach().double().norm()))
        out_d[pre + "grad_names"] = np.array(names)
        out_d[pre + "grad_norm"] = np.array(gn)
        out_d[pre + "grad_is_none"] = np.array(isnone, dtype=np.int8)
        opt.step()  # :154
        ps, ss = [], []
        for n, p in model.named_parameters():
            ps.append(mg._summ(p))
            state = opt.state.get(p, {})
            ss.append(np.stack([mg._summ(state[k]) if k in state else np.zeros(2) for k in STATE_KEYS[kind]]))
        out_d[pre + "param_sums"] = np.stack(ps)            # [tensor][sum, sum|.|]
        out_d[pre + "state_sums"] = np.stack(ss)            # [tensor][state key][sum, sum|.|]
        for n, b in model.named_buffers():
            if "relative_position_index" in n or "attn_mask" in n:
                continue
            out_d[pre + "buf." + n] = b.detach().numpy().copy()
    out_d["state_keys"] = np.array(STATE_KEYS[kind])
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out_d)
    print(name, "loss_f", out_d[f"s{steps - 1}.loss_f"], "total_norm", out_d[f"s{steps - 1}.total_norm"],
          os.path.getsize(path), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--float64", metavar="DIR", default=None,
                    help="run the same cases with the model and inputs in float64 and write them to DIR (not goldens: the "
                         "reference's own float32-vs-float64 spread, tools/optim_golden_spread.py --against DIR)")
    a = ap.parse_args()
    bm, bb, fm = mg._import_reference()
    tiny = dict(dataset="CREMAD", spec_hw=(65, 47), frames=2, batch=4, alpha=4.0, steps=3)
    if a.float64:
        os.makedirs(a.float64, exist_ok=True)
        tiny.update(dtype=torch.float64, out_dir=a.float64)
    cases = {
        "dgl_adamw_tiny_b4": lambda: run_optim_case("dgl_adamw_tiny_b4", bm, bb, fm, "Adam", image_hw=(64, 64), **tiny),
        "dgl_adagrad_tiny_b4": lambda: run_optim_case("dgl_adagrad_tiny_b4", bm, bb, fm, "AdaGrad", image_hw=(64, 64), **tiny),
        "dgl_swin_adamw_tiny_b4": lambda: run_optim_case("dgl_swin_adamw_tiny_b4", bm, bb, fm, "Adam", image_hw=(56, 56),
                                                         swin_cfg=fx.SWIN_TINY2, **tiny),
    }
    for k, f in cases.items():
        if a.only and a.only not in k:
            continue
        f()


if __name__ == "__main__":
    main()
