#!/usr/bin/env python3
"""Golden vectors of alternating unimodal training on a shared head (MLA), generated as the literal torch
CPU float32 loop on the reference's own parts like make_golden_unimodal.py does:
    python tests/golden/make_golden_mla.py            # writes mla_plain_tiny_b4.npz, mla_gs_tiny_b4.npz
    python tests/golden/make_golden_mla.py --spread   # writes nothing: the loop's float32-vs-float64 spread

The model is the reference's `resnet18('audio')`, `resnet18('visual')` and one `nn.Linear(512, 6)` with the pooling glue of its
basic_model.py:73-82; the state is loaded by name (`fx.model_state(6, "concat_dgl")` for the encoders, `fx.make_state` for
classifier.weight / classifier.bias).  A batch is two half-steps, audio then visual, each
    opt.zero_grad(set_to_none=True); out = classifier(pool(net(x))); CrossEntropyLoss(out, label).backward()
    [shaping, from the second half-step on:  k = P r_prev; P -= outer(k, k) / (alpha + r_prev . k); P /= ||P||_F;
                                            classifier.weight.grad = classifier.weight.grad @ P.T]
    r_prev = the pooled feature's mean over the batch;  clip_grad_norm_(this half-step's tensors, 40);  opt.step()
with ONE SGD(momentum .9, wd 1e-4) over all parameters: a parameter whose .grad is None is skipped, so the idle encoder sees no
weight decay and no momentum drift.  `mla_plain_tiny_b4` runs with shaping off, `mla_gs_tiny_b4` with shaping on, normalize on
and alpha = 0.1 ** (1 + step / 2) (gdl.mla_alpha with two steps per epoch).  Two batches = four half-steps.

The record per half-step is make_golden_unimodal.run_unimodal_step_case's under the prefix s<batch>.<a|v>. (float64 norm of the
float32 gradients for the clip, per-tensor norms BEFORE the clip, everything else of the clipped gradients, over ALL named
parameters with grad_is_none = 1 for the idle encoder's), plus
  r            the pooled feature's mean [512] (what the NEXT half-step shapes against)
  shaped       1 if this half-step's classifier.weight.grad went through P
  P16, Pdiag, Prowsum, Pfro   of P after this half-step: P[:16, :16], its diagonal, its float64 row sums and Frobenius norm (P
               itself is 1 MB: too large to commit whole)
  alpha        the half-step's alpha_s
"""
import argparse
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (puts the repository root on sys.path)
import make_golden_joint as mgj  # noqa: E402
import mla_ref  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import fixtures as fx  # noqa: E402

MAX_NORM = mgj.MAX_NORM
TINY = ("CREMAD", (65, 47), 2, (64, 64), 4)
STEPS_PER_EPOCH = 2


class _SharedHeadAV(nn.Module):
    def __init__(self, bb, n_classes, batch):
        super().__init__()
        args = argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", batch_size=batch)
        self.audio_net = bb.resnet18(modality="audio", args=args)
        self.visual_net = bb.resnet18(modality="visual", args=args)
        self.classifier = nn.Linear(512, n_classes)

    def feature(self, m, x):
        if m == "audio":
            return torch.flatten(F.adaptive_avg_pool2d(self.audio_net(x), 1), 1)
        B = x.shape[0]
        v = self.visual_net(x)
        _, C, H, W = v.size()
        return torch.flatten(F.adaptive_avg_pool3d(v.view(B, -1, C, H, W).permute(0, 2, 1, 3, 4), 1), 1)


def mla_state(n_classes):
    ps, bs = fx.model_state(n_classes, "concat_dgl")
    keep = ("audio_net.", "visual_net.")
    P = {k: v for k, v in ps.items() if k.startswith(keep)}
    P.update(fx.make_state({"classifier.weight": (n_classes, 512), "classifier.bias": (n_classes,)}))
    return P, {k: v for k, v in bs.items() if k.startswith(keep)}


def run_mla_case(name, bb, shaping, dataset, spec_hw, frames, image_hw, batch, steps, seed=0, lr=2e-3, dtype=torch.float32,
                 save=True):
    torch.manual_seed(0)
    torch.set_num_threads(8)
    n_classes = fx.N_CLASSES[dataset]
    model = _SharedHeadAV(bb, n_classes, batch)
    ps, bs = mla_state(n_classes)
    names = [n for n, _ in model.named_parameters()]
    assert names == list(ps), "parameter order differs from mla_state's"
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in {**ps, **bs}.items()}, strict=True)
    model = model.to(dtype)
    opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
    crit = nn.CrossEntropyLoss()
    cfg = dict(name=name, dataset=dataset, n_classes=n_classes, spec_hw=list(spec_hw), frames=frames, image_hw=list(image_hw),
               batch=batch, steps=steps, mode="mla", shaping=bool(shaping), normalize=True, steps_per_epoch=STEPS_PER_EPOCH,
               seed=seed, lr=lr, momentum=0.9, weight_decay=1e-4, max_norm=MAX_NORM, torch=torch.__version__)
    out_d = {"config": np.array(json.dumps(cfg)), "param_names": np.array(names)}
    P = torch.eye(512, dtype=dtype)
    r_prev = None
    model.train()
    for st in range(steps):
        spec, image, label = fx.make_batch(seed + st, batch, spec_hw, frames, image_hw, n_classes)
        spec, image, label = torch.from_numpy(spec), torch.from_numpy(image), torch.from_numpy(label)
        alpha = mla_ref.mla_alpha(st, STEPS_PER_EPOCH)
        for m in ("audio", "visual"):
            pre = f"s{st}.{m[0]}."
            opt.zero_grad(set_to_none=True)
            feat = model.feature(m, (spec.unsqueeze(1) if m == "audio" else image).to(dtype))
            out = model.classifier(feat)
            loss = crit(out, label)
            loss.backward()
            shaped = bool(shaping and r_prev is not None)
            if shaped:
                with torch.no_grad():
                    a = torch.tensor(np.float32(alpha).item(), dtype=dtype)
                    k = P @ r_prev
                    P = P - torch.outer(k, k) / (a + torch.dot(r_prev, k))
                    P = P / torch.norm(P)
                    model.classifier.weight.grad = model.classifier.weight.grad @ P.t()
            r_prev = feat.detach().mean(dim=0)
            out_d[pre + "out"] = out.detach().numpy()
            out_d[pre + "loss_f"] = np.float64(loss.item())
            out_d[pre + "r"] = r_prev.numpy().copy()
            out_d[pre + "shaped"] = np.int8(shaped)
            out_d[pre + "alpha"] = np.float64(alpha)
            for kk, vv in mla_ref.p_summary(P.numpy()).items():
                out_d[pre + kk] = vv
            params = list(model.named_parameters())
            none = [p.grad is None for _, p in params]
            idle = ("visual_net." if m == "audio" else "audio_net.")
            assert [n for (n, _), x in zip(params, none) if x] == [n for n in names if n.startswith(idle)]
            live = [p for p in model.parameters() if p.grad is not None]
            gn = [0.0 if p.grad is None else mgj._norm64(p.grad) for _, p in params]  # before the clip
            total = float(np.sqrt(sum(v * v for v in gn)))
            t32 = torch.norm(torch.stack([torch.norm(p.grad.detach(), 2) for p in live]), 2)  # clip_grad_norm_'s own sum
            out_d[pre + "total_norm"] = np.float64(total)
            out_d[pre + "total_norm_torch32"] = np.float64(t32.item())
            coef = min(1.0, MAX_NORM / (total + 1e-6))
            if coef < 1.0:
                for p in live:
                    p.grad.mul_(coef)
            enc_sum = sum(torch.abs(p.grad).mean().item() for p in getattr(model, m + "_net").parameters())
            out_d[pre + "audio_grad_sum"] = np.float64(enc_sum if m == "audio" else 0.0)
            out_d[pre + "visual_grad_sum"] = np.float64(enc_sum if m == "visual" else 0.0)
            gam, gh8 = [], []
            for n, p in params:
                if p.grad is None:
                    gam.append(0.0)
                    gh8.append(np.zeros(8, dtype=out_d[pre + "out"].dtype))
                    continue
                g = p.grad.detach()
                gam.append(float(g.abs().double().mean()))
                h = g.flatten()[:8].numpy()
                gh8.append(np.pad(h, (0, 8 - len(h))))
                if g.numel() <= 10000:
                    out_d[pre + "grad." + n] = g.numpy().copy()
            out_d[pre + "grad_names"] = np.array(names)
            out_d[pre + "grad_norm"] = np.array(gn)
            out_d[pre + "grad_absmean"] = np.array(gam)
            out_d[pre + "grad_head8"] = np.stack(gh8)
            out_d[pre + "grad_is_none"] = np.array(none, dtype=np.int8)
            opt.step()
            psum, ph8, ms = [], [], []
            for n, p in params:
                psum.append(mg._summ(p))
                h = p.detach().flatten()[:8].numpy()
                ph8.append(np.pad(h, (0, 8 - len(h))))
                ms.append(mg._summ(opt.state[p]["momentum_buffer"]) if p in opt.state and "momentum_buffer" in opt.state[p]
                          else np.zeros(2))
            out_d[pre + "param_sums"] = np.stack(psum)
            out_d[pre + "param_head8"] = np.stack(ph8)
            out_d[pre + "momentum_sums"] = np.stack(ms)
            for n, b in model.named_buffers():
                out_d[pre + "buf." + n] = b.detach().numpy().copy()
            print(name, "batch", st, m, "loss", loss.item(), "total_norm", total, "torch32", t32.item(), "shaped", shaped)
    model.eval()
    with torch.no_grad():
        spec, image, label = fx.make_batch(seed + 1000, batch, spec_hw, frames, image_hw, n_classes)
        out_d["eval.out_a"] = model.classifier(model.feature("audio", torch.from_numpy(spec).unsqueeze(1).to(dtype))).numpy()
        out_d["eval.out_v"] = model.classifier(model.feature("visual", torch.from_numpy(image).to(dtype))).numpy()
    if not save:
        return out_d
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out_d)
    print(name, "ok", os.path.getsize(path), "bytes")


def spread(name, bb, shaping, steps):
    """The float32 fixture `name` (as committed) against the same loop in float64 (docs/parity_log.md)."""
    g = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
    d = run_mla_case(name, bb, shaping, *TINY, steps=steps, dtype=torch.float64, save=False)
    for st in range(steps):
        for m in "av":
            pre = f"s{st}.{m}."
            live = g[pre + "grad_is_none"] == 0
            gn32, gn64 = g[pre + "grad_norm"][live], d[pre + "grad_norm"][live]
            print(f"spread {name} {pre} logits {np.abs(g[pre + 'out'] - d[pre + 'out']).max():.2e}  per-tensor norm "
                  f"{np.max(np.abs(gn32 - gn64) / gn64):.2e}  total_norm {float(g[pre + 'total_norm']):.4f} / "
                  f"{float(d[pre + 'total_norm']):.4f}  loss {float(g[pre + 'loss_f']):.6f} / {float(d[pre + 'loss_f']):.6f}  "
                  f"r {np.abs(g[pre + 'r'] - d[pre + 'r']).max():.2e}  P16 {np.abs(g[pre + 'P16'] - d[pre + 'P16']).max():.2e}")
    for k in ("eval.out_a", "eval.out_v"):
        print(f"spread {name} {k} {np.abs(g[k] - d[k]).max():.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--spread", action="store_true", help="write nothing: print the float32-vs-float64 spread of the fixtures")
    a = ap.parse_args()
    _, bb, _ = mg._import_reference()
    for name, shaping in (("mla_plain_tiny_b4", False), ("mla_gs_tiny_b4", True)):
        if a.only and a.only not in name:
            continue
        if a.spread:
            spread(name, bb, shaping, 2)
        else:
            run_mla_case(name, bb, shaping, *TINY, steps=2)


if __name__ == "__main__":
    main()
