#!/usr/bin/env python3
"""Golden vectors of the probabilistic-embedding branch (main.py --pe 1 --beta b), generated on the CPU against the imported
reference encoders like make_golden_joint.py:
    python tests/golden/make_golden_dul.py      # writes dul_uni_audio_tiny_b4.npz, dul_joint_concat_tiny_b4.npz,
                                                #        dul_joint_concat_beta2_tiny_b4.npz, dul_mtl_sum_tiny_b4.npz

The model is the reference's `resnet18` twice (or once) with the two stacks of models/swin_transformer.py:574-582 registered
behind layer4 under the reference's names -- nn.Conv2d(512, 512, 1) + nn.BatchNorm2d(512), `mu_dul_backbone` and
`logvar_dul_backbone` -- the forward of :643-667 with the noise INJECTED (tests/dul_ref.py's generator, seed 5, step = the step
index, so that the runner's `pe_eps` reproduces it), the pooling glue of basic_model.py:73-82, `regurize` of main.py:92-102 and
loss = loss_cls + (regurize_a + regurize_v) * beta (main.py:191-213); clip_grad_norm_(.., 40), SGD(momentum .9, wd 1e-4).
Cases at the tiny fixture shapes (spec 65 x 47, frames 64 x 64), B = 4, two steps each:
    dul_uni_audio_tiny_b4        the audio encoder alone + Linear(512, 6), T = 1, beta 1e-5
    dul_joint_concat_tiny_b4     ConcatFusion, loss_cls = CE(out), T = 3, beta 1e-5
    dul_joint_concat_beta2_...   the same with beta 1e-2 (the KL gradient is not below the comparison's resolution)
    dul_mtl_sum_tiny_b4          SumFusion_DGL undetached, loss_cls = CE(out) + 2.5 (CE(out_a) + CE(out_v)), T = 3, beta 1e-5
The record is make_golden_joint.run_joint_step_case's, plus s<k>.reg_a / reg_v, s<k>.loss_a / loss_v where they exist.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (puts the repository root on sys.path)
import make_golden_ablation as mga  # noqa: E402
import make_golden_joint as mgj  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import dul_ref as dr  # noqa: E402
from oracle import fixtures as fx  # noqa: E402

MAX_NORM = mgj.MAX_NORM
EPS_SEED = 5
GAMMA = 2.5


def regurize(mul, std):
    """main.py:92-102"""
    variance_dul = (std ** 2).view(std.shape[0], -1)
    mul = mul.view(mul.shape[0], -1)
    loss_kl = (variance_dul + mul ** 2 - torch.log(variance_dul + 1e-8) - 1) * 0.5
    return torch.mean(torch.sum(loss_kl, dim=1))


def add_stacks(net):
    net.mu_dul_backbone = nn.Sequential(nn.Conv2d(512, 512, kernel_size=1, stride=1, padding=0), nn.BatchNorm2d(512))
    net.logvar_dul_backbone = nn.Sequential(nn.Conv2d(512, 512, kernel_size=1, stride=1, padding=0), nn.BatchNorm2d(512))
    return net


def branch(net, fmap, step, modality):
    """swin_transformer.py:643-667 on the ResNet's map, the noise injected: (out map, mu, sd)"""
    mu = net.mu_dul_backbone(fmap)
    sd = (net.logvar_dul_backbone(fmap) * 0.5).exp()
    if not net.training:
        return mu, mu, sd
    n, c, h, w = fmap.shape
    eps = torch.from_numpy(dr.golden_eps(n, h * w, EPS_SEED, step, modality)).view(n, h, w, c).permute(0, 3, 1, 2).to(fmap.dtype)
    return mu + eps * sd, mu, sd


class _PeAV(nn.Module):
    def __init__(self, bb, fm, n_classes, kind, fusion):
        super().__init__()
        self.kind = kind
        if kind == "unimodal":
            self.audio_net = add_stacks(bb.resnet18(modality="audio", args=None))
            self.audio_classifier = nn.Linear(512, n_classes)
            return
        self.fusion_module = fm.ConcatFusion(output_dim=n_classes) if kind == "joint" else \
            {"concat": fm.ConcatFusion_DGL, "sum": fm.SumFusion_DGL}[fusion](output_dim=n_classes)
        self.audio_net = add_stacks(bb.resnet18(modality="audio", args=None))
        self.visual_net = add_stacks(bb.resnet18(modality="visual", args=None))

    def forward(self, audio, visual, step):
        a, mu_a, sd_a = branch(self.audio_net, self.audio_net(audio), step, dr.AUDIO)
        B = a.size()[0]
        a = torch.flatten(F.adaptive_avg_pool2d(a, 1), 1)
        if self.kind == "unimodal":
            return (self.audio_classifier(a),), regurize(mu_a, sd_a), None
        v, mu_v, sd_v = branch(self.visual_net, self.visual_net(visual), step, dr.VISUAL)
        (_, C, H, W) = v.size()
        v = torch.flatten(F.adaptive_avg_pool3d(v.view(B, -1, C, H, W).permute(0, 2, 1, 3, 4), 1), 1)
        if self.kind == "joint":
            outs = (self.fusion_module(a, v)[2],)
        else:
            a_out, v_out, out = mga.undetached_head(self.fusion_module, a, v)
            outs = (out, a_out, v_out)
        return outs, regurize(mu_a, sd_a), regurize(mu_v, sd_v)


def state_of(model, n_classes, kind, fusion):
    ps, bs = fx.model_state(n_classes, fusion + "_dgl")
    P, Bf = {}, {}
    for n, _ in model.named_parameters():
        if n in ps:
            P[n] = ps[n]
    for pre in ("audio_net.", "visual_net."):
        if hasattr(model, pre[:-1]):
            dp, db = dr.dul_state(pre)
            P.update(dp)
            Bf.update({k: v for k, v in bs.items() if k.startswith(pre)})
            Bf.update(db)
    if kind == "unimodal":
        P.update(fx.make_state({"audio_classifier.weight": (n_classes, 512), "audio_classifier.bias": (n_classes,)}))
    return P, Bf


def run_case(name, bb, fm, kind, fusion, frames, beta, steps=2, seed=0, lr=2e-3, batch=4, spec_hw=(65, 47), image_hw=(64, 64),
             dataset="CREMAD"):
    torch.manual_seed(0)
    torch.set_num_threads(8)
    n_classes = fx.N_CLASSES[dataset]
    model = _PeAV(bb, fm, n_classes, kind, fusion)
    P, Bf = state_of(model, n_classes, kind, fusion)
    assert sorted(P) == sorted(n for n, _ in model.named_parameters())
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in {**P, **Bf}.items()}, strict=True)
    opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
    crit = nn.CrossEntropyLoss()
    cfg = dict(name=name, dataset=dataset, n_classes=n_classes, spec_hw=list(spec_hw), frames=frames, image_hw=list(image_hw),
               batch=batch, alpha=GAMMA if kind == "mtl" else 0.0, steps=steps, mode=kind, seed=seed, lr=lr, momentum=0.9,
               weight_decay=1e-4, max_norm=MAX_NORM, torch=torch.__version__, fusion=fusion, beta=beta, eps_seed=EPS_SEED)
    out_d = {"config": np.array(json.dumps(cfg))}
    model.train()
    for st in range(steps):
        spec, image, label = fx.make_batch(seed + st, batch, spec_hw, frames, image_hw, n_classes)
        spec, image, label = torch.from_numpy(spec), torch.from_numpy(image), torch.from_numpy(label)
        opt.zero_grad()
        pre = f"s{st}."
        outs, reg_a, reg_v = model(spec.unsqueeze(1), image, st)
        loss_f = crit(outs[0], label)
        loss = loss_f
        if kind == "mtl":
            loss_a, loss_v = crit(outs[1], label), crit(outs[2], label)
            loss = loss + GAMMA * (loss_a + loss_v)
            out_d.update({pre + "out_a": outs[1].detach().numpy(), pre + "out_v": outs[2].detach().numpy(),
                          pre + "loss_a": np.float64(loss_a.item()), pre + "loss_v": np.float64(loss_v.item())})
        loss = loss + (reg_a + (reg_v if reg_v is not None else 0.0)) * beta
        loss.backward()
        out_d[pre + "out"] = outs[0].detach().numpy()
        out_d[pre + "loss_f"] = np.float64(loss_f.item())
        out_d[pre + "reg_a"] = np.float64(reg_a.item())
        if reg_v is not None:
            out_d[pre + "reg_v"] = np.float64(reg_v.item())
        params = list(model.named_parameters())
        assert all(p.grad is not None for _, p in params)
        gn = [mgj._norm64(p.grad) for _, p in params]  # before the clip
        total = float(np.sqrt(sum(v * v for v in gn)))
        out_d[pre + "total_norm"] = np.float64(total)
        coef = min(1.0, MAX_NORM / (total + 1e-6))
        if coef < 1.0:
            for _, p in params:
                p.grad.mul_(coef)
        out_d[pre + "audio_grad_sum"] = np.float64(sum(torch.abs(p.grad).mean().item() for p in model.audio_net.parameters()))
        if kind != "unimodal":
            out_d[pre + "visual_grad_sum"] = np.float64(sum(torch.abs(p.grad).mean().item() for p in model.visual_net.parameters()))
        out_d[pre + "grad_names"] = np.array([n for n, _ in params])
        out_d[pre + "grad_norm"] = np.array(gn)
        opt.step()
        out_d[pre + "param_sums"] = np.stack([mg._summ(p) for _, p in params])
        for n, b in model.named_buffers():
            if "_dul_" in n:
                out_d[pre + "buf." + n] = b.detach().numpy().copy()
        print(name, "step", st, "loss_f", loss_f.item(), "reg_a", reg_a.item(), "reg_v", None if reg_v is None else reg_v.item(),
              "total_norm", total)
    model.eval()
    with torch.no_grad():
        spec, image, label = fx.make_batch(seed + 1000, batch, spec_hw, frames, image_hw, n_classes)
        out_d["eval.out"] = model(torch.from_numpy(spec).unsqueeze(1), torch.from_numpy(image), 0)[0][0].numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out_d)
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    bm, bb, fm = mg._import_reference()
    run_case("dul_uni_audio_tiny_b4", bb, fm, "unimodal", "concat", 1, 1e-5)
    run_case("dul_joint_concat_tiny_b4", bb, fm, "joint", "concat", 3, 1e-5)
    run_case("dul_joint_concat_beta2_tiny_b4", bb, fm, "joint", "concat", 3, 1e-2)
    run_case("dul_mtl_sum_tiny_b4", bb, fm, "mtl", "sum", 3, 1e-5)


if __name__ == "__main__":
    main()
