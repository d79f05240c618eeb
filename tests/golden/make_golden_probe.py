#!/usr/bin/env python3
"""Golden vectors of the LINEAR PROBE (gdl.extract_features + gdl.LinearProbe), generated on the CPU by importing the reference
like make_golden_unimodal.py does:
    python tests/golden/make_golden_probe.py            # writes probe_audio_tiny.npz, probe_visual_tiny.npz

The encoder is the reference's own `resnet18` with `fx.model_state(6, "concat_dgl")`'s audio_net / visual_net entries loaded --
BatchNorm running statistics that are not the constructor's 0 / 1, which is what makes eval mode a real test -- run in eval()
on 3 batches of 4 from `fx.make_batch(seed 0 .. 2)` at the tiny shapes, followed by the pooling of basic_model.py:73-82
(adaptive_avg_pool2d of the audio map; the visual maps regrouped per sample and adaptive_avg_pool3d).  On the 12 pooled
features a torch float32 probe is trained for 3 epochs at B = 4, n = 6: nn.Linear + CrossEntropyLoss + clip_grad_norm_ +
optim.SGD(momentum .9, weight_decay 1e-4), the scripts' step without the encoder (tests/probe_ref.torch_fit).  Keys:
  features [12, 512], labels [12]
  W0 [6, 512], b0 [6]          nn.init.xavier_normal_ on a generator seeded 0 / zeros: gdl.LinearProbe(6, dev, seed=0)'s start
  order [3, 3, 4] int32        gdl.probe_order(12, 4, 3, <the same generator, after W0>): what fit(order=None) draws
  <run>.e<k>.W / b / mW / mb / loss / norms   after epoch k = 0 .. 2; run `n40` at max_norm 40 (never clips), `clip` at
                               max_norm CLIP (every step clips: asserted here, otherwise the clip branch is untested)
  config                       JSON: lr, momentum, weight_decay, the two max_norms, torch version
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
import probe_ref  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import fixtures as fx  # noqa: E402

SPEC_HW, FRAMES, IMAGE_HW, BATCH = (65, 47), 2, (64, 64), 4  # the shapes of every tiny step fixture
N_CLASSES, N_BATCHES, EPOCHS = 6, 3, 3
LR, MOMENTUM, WEIGHT_DECAY, MAX_NORM, CLIP = 1e-2, 0.9, 1e-4, 40.0, 0.05


def pooled_features(bb, modality):
    net = bb.resnet18(modality=modality, args=None)
    ps, bs = fx.model_state(N_CLASSES, "concat_dgl")
    pre = modality + "_net."
    sd = {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in {**ps, **bs}.items() if k.startswith(pre)}
    net.load_state_dict(sd, strict=True)
    net.eval()
    feats, labels = [], []
    with torch.no_grad():
        for seed in range(N_BATCHES):
            spec, image, label = fx.make_batch(seed, BATCH, SPEC_HW, FRAMES, IMAGE_HW, N_CLASSES)
            if modality == "audio":
                f = F.adaptive_avg_pool2d(net(torch.from_numpy(spec).unsqueeze(1)), 1)
            else:
                v = net(torch.from_numpy(image))
                _, C, H, W = v.shape
                f = F.adaptive_avg_pool3d(v.view(BATCH, -1, C, H, W).permute(0, 2, 1, 3, 4), 1)
            feats.append(torch.flatten(f, 1).numpy())
            labels.append(label)
    for k, v in net.state_dict().items():  # eval(): nothing moved
        assert torch.equal(v, sd[k]), k
    return np.concatenate(feats).astype(np.float32), np.concatenate(labels).astype(np.int64)


def run_case(name, bb, modality):
    torch.manual_seed(0)
    torch.set_num_threads(8)
    feats, labels = pooled_features(bb, modality)
    gen = torch.Generator()
    gen.manual_seed(0)
    W0 = torch.empty((N_CLASSES, 512))
    torch.nn.init.xavier_normal_(W0, generator=gen)
    W0, b0 = W0.numpy(), np.zeros(N_CLASSES, dtype=np.float32)
    n, steps = feats.shape[0], feats.shape[0] // BATCH
    order = np.stack([torch.randperm(n, generator=gen)[:steps * BATCH].view(steps, BATCH).numpy() for _ in range(EPOCHS)])
    order = order.astype(np.int32)
    cfg = dict(name=name, modality=modality, n_classes=N_CLASSES, batch=BATCH, epochs=EPOCHS, lr=LR, momentum=MOMENTUM,
               weight_decay=WEIGHT_DECAY, max_norm=MAX_NORM, clip_norm=CLIP, spec_hw=list(SPEC_HW), frames=FRAMES,
               image_hw=list(IMAGE_HW), torch=torch.__version__)
    d = {"config": np.array(json.dumps(cfg)), "features": feats, "labels": labels, "W0": W0, "b0": b0, "order": order}
    for run, mn in (("n40", MAX_NORM), ("clip", CLIP)):
        traj = probe_ref.torch_fit(feats, labels, order, W0, b0, lr=LR, mu=MOMENTUM, wd=WEIGHT_DECAY, max_norm=mn)
        norms = np.concatenate([t["norms"] for t in traj])
        if run == "clip":
            assert (norms > CLIP).all(), ("a step of the clip run did not clip", norms.min())
        else:
            assert (norms < MAX_NORM).all(), ("a step of the max_norm = 40 run clipped", norms.max())
        for e, t in enumerate(traj):
            for k in ("W", "b", "mW", "mb"):
                d[f"{run}.e{e}.{k}"] = t[k].astype(np.float32)
            d[f"{run}.e{e}.loss"] = np.float64(t["loss"])
            d[f"{run}.e{e}.norms"] = t["norms"].astype(np.float64)
        print(name, run, "losses", [round(t["loss"], 5) for t in traj], "norms %.3g .. %.3g" % (norms.min(), norms.max()))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **d)
    print(name, "ok", os.path.getsize(path), "bytes; mean |feature|", float(np.abs(feats).mean()))


def main():
    _, bb, _ = mg._import_reference()
    for name, modality in (("probe_audio_tiny", "audio"), ("probe_visual_tiny", "visual")):
        run_case(name, bb, modality)


if __name__ == "__main__":
    main()
