"""Linear probe of a frozen encoder: the one number per encoder that this line of work compares encoders by (OGM-GE; the DGL
paper's multimodally-trained against alone-trained encoders) -- freeze the encoder in eval mode (BatchNorm running statistics),
take its pooled 512-wide feature, train a fresh `Linear(512, n_classes)` on it, report that classifier's test accuracy.

    bank = gdl.extract_features(model, 'audio', train_batches)         # [N, 512] float32 + [N] int64, on the device
    probe = gdl.LinearProbe(n_classes, device, seed=0)
    losses = probe.fit(bank, epochs=100, lr=[gdl.multistep_lr(1e-3, [70], 0.1, e) for e in range(100)])
    acc, counts = probe.score(gdl.extract_features(model, 'audio', test_batches))

The features never leave the device, and the fit is one C call per epoch (gdl_linprobe_epoch, csrc/linprobe.hip): the step is
main.py's unimodal step with the encoder removed -- mean cross-entropy, clip_grad_norm_ over {dW, db}, SGD with momentum and
weight decay -- on the rows an index table names.  A whole fit costs one upload (the table), one synchronisation and one host
copy (the epoch losses).  Augmented features: re-extract per epoch and call `fit(epochs=1)` repeatedly; the probe keeps its
state between calls.

The probe is not one of the reference's scripts: its arithmetic is the scripts' own unimodal step on frozen features.  ResNet18
encoders only (no Swin branch: 768 features), one device (no process group).
"""
import math

import numpy as np
import torch

from . import _lib as L
from .encoder import EncoderEngine

FEAT = 512
MAX_CLASSES = 512


def multistep_lr(lr0, milestones, ratio, epoch):
    """The learning rate the scripts train epoch `epoch` (0-based) with: `MultiStepLR(optimizer, milestones, ratio)` whose
    `scheduler.step()` runs at the TOP of train_epoch (main_dgl.py:73-74), before any optimizer step -- so epoch e trains after
    e + 1 scheduler steps and a milestone m takes effect from epoch m - 1 on.  The product is built as the scheduler builds it
    (lr *= ratio ** multiplicity, milestones ascending): the same float."""
    if epoch < 0:
        raise ValueError(f"multistep_lr: epoch must be >= 0, got {epoch}")
    lr = float(lr0)
    ms = sorted(int(m) for m in milestones)
    for m in sorted(set(ms)):
        if 1 <= m <= epoch + 1:  # (last_epoch = 0 is the scheduler's construction: a milestone 0 never fires)
            lr = lr * float(ratio) ** ms.count(m)
    return lr


def probe_order(n, batch_size, epochs, generator):
    """The fit's index table [epochs, n // batch_size, batch_size] int32 (host): per epoch one `torch.randperm(n)` on
    `generator`, its ragged tail dropped as the scripts' `drop_last=True` drops it."""
    if batch_size < 1 or n < batch_size:
        raise L.GdlError(f"LinearProbe: batch_size must be in [1, N = {n}], got {batch_size}")
    steps = n // batch_size
    tab = torch.empty((epochs, steps, batch_size), dtype=torch.int32)
    for e in range(epochs):
        tab[e] = torch.randperm(n, generator=generator)[:steps * batch_size].view(steps, batch_size).to(torch.int32)
    return tab


def check_order(order, n, epochs, batch_size):
    """A caller's index table as the fit uploads it (int32, host, contiguous): an integer [epochs, steps, batch_size] array or
    tensor whose entries are rows of a bank of n; anything else is refused here, on the host, before a launch."""
    tab = torch.as_tensor(np.asarray(order.cpu() if torch.is_tensor(order) else order))
    if tab.dim() != 3 or tab.shape[0] != epochs or tab.shape[2] != batch_size or tab.dtype.is_floating_point or tab.dtype == torch.bool:
        raise L.GdlError(f"LinearProbe.fit: order must be an integer [epochs = {epochs}, steps, batch_size = {batch_size}] table, "
                         f"got {tab.dtype} {tuple(tab.shape)}")
    if tab.numel() and (int(tab.min()) < 0 or int(tab.max()) >= n):
        raise L.GdlError(f"LinearProbe.fit: order holds an index outside [0, N = {n}) (min {int(tab.min())}, max {int(tab.max())})")
    return tab.to(torch.int32).contiguous()


class FeatureBank:
    """`features` [N, 512] float32 and `labels` [N] int64, both on the device; `modality` is where they came from."""

    def __init__(self, features, labels, modality=None):
        if features.dim() != 2 or features.shape[1] != FEAT or features.dtype != torch.float32 or not features.is_contiguous():
            raise L.GdlError(f"FeatureBank: features must be a contiguous float32 [N, {FEAT}] tensor, got {features.dtype} "
                             f"{tuple(features.shape)}")
        if labels.dtype != torch.int64 or tuple(labels.shape) != (features.shape[0],) or labels.device != features.device:
            raise L.GdlError(f"FeatureBank: labels must be an int64 [N = {features.shape[0]}] tensor on {features.device}")
        self.features, self.labels, self.modality = features, labels.contiguous(), modality

    @property
    def N(self):
        return self.features.shape[0]

    def __len__(self):
        return self.features.shape[0]

    @property
    def device(self):
        return self.features.device


def _encoder_of(model, modality):
    if modality not in ("audio", "visual"):
        raise L.GdlError(f"extract_features: modality must be 'audio' or 'visual', got {modality!r}")
    net = getattr(model, modality + "_net", None)
    if net is None:
        raise L.GdlError(f"extract_features: the model has no {modality}_net (modality = {getattr(model, 'modality', None)!r})")
    if hasattr(net, "cfg") and hasattr(net, "num_features"):
        raise L.GdlError(f"extract_features: the Swin branch ({int(net.num_features)} features) is not built for the linear probe "
                         f"(ResNet18 encoders, {FEAT} features)")
    if getattr(net, "pe", False):
        raise L.GdlError("extract_features: the probabilistic-embedding branch (args.pe) is not built for the linear probe")
    if not hasattr(net, "_bn_layers") or len(list(net.parameters())) != L.ENC_NPARAMS:
        raise L.GdlError(f"extract_features: {modality}_net must be the ResNet18 mirror (60 tensors)")
    return net


def extract_features(model, modality, batches, dtype=None):
    """The pooled features of `model`'s frozen `modality` encoder over `batches` of (spec [B,F,T'], image [B,3,T,H,W], label [B]
    int64) as for `valid()` -- the other modality's tensor may be None -- as a FeatureBank on the model's device.  Each batch is
    one eval-mode `EncoderEngine.forward(x, False, feat_out=<its rows of the bank>)` on the current stream: no host copy, no
    synchronisation.  A batch of another size (the last one) re-plans the engine.  The encoder's parameters and BatchNorm
    buffers are only read.  dtype: the engine's storage type ('bf16' / 'f32'), default the encoder's own `gdl_dtype`."""
    net = _encoder_of(model, modality)
    device = next(net.parameters()).device
    if device.type != "cuda":
        raise L.GdlError("extract_features: the model must live on an MI355X (cuda) device; there is no CPU path")
    dtype = dtype if dtype is not None else net.gdl_dtype
    items = []
    for spec, image, label in batches:
        x = spec if modality == "audio" else image
        want = "spec [B,F,T']" if modality == "audio" else "image [B,3,T,H,W]"
        if x is None or x.dim() != (3 if modality == "audio" else 5) or (modality == "visual" and x.shape[1] != 3):
            raise L.GdlError(f"extract_features: the {modality} encoder takes {want}")
        if x.device != device or label.device != device:
            raise L.GdlError(f"extract_features: the batches must be on {device}")
        if label.dtype != torch.int64 or tuple(label.shape) != (x.shape[0],):
            raise L.GdlError(f"extract_features: label must be an int64 [B = {x.shape[0]}] tensor")
        items.append((x.unsqueeze(1) if modality == "audio" else x, label))
    n = sum(x.shape[0] for x, _ in items)
    if n == 0:
        raise L.GdlError("extract_features: no batches")
    with torch.cuda.device(device):
        feats = torch.empty((n, FEAT), device=device)
        labels = torch.empty(n, dtype=torch.int64, device=device)
        bns = net._bn_layers()
        eng, key, o = None, None, 0
        for x, label in items:
            if tuple(x.shape) != key:
                key = tuple(x.shape)
                T, H, W = (1, x.shape[2], x.shape[3]) if modality == "audio" else tuple(x.shape[2:])
                eng = EncoderEngine(modality, dtype, x.shape[0], T, H, W, device)
                eng.set_params([p.data for p in net.parameters()], [b.running_mean for b in bns], [b.running_var for b in bns],
                               [b.num_batches_tracked for b in bns])
            B = x.shape[0]
            eng.forward(x, False, feat_out=feats[o:o + B])
            labels[o:o + B].copy_(label, non_blocking=True)
            o += B
    return FeatureBank(feats, labels, modality)


class LinearProbe:
    """A fresh `Linear(512, n_classes)` trained on a FeatureBank by the fused fit.  `weight` / `bias` start as the mirror's
    `utils.weight_init` leaves a Linear (Xavier-normal weight, zero bias), drawn from a generator seeded by `seed`; the same
    generator draws the epochs' permutations."""

    def __init__(self, n_classes, device, seed=0):
        n_classes = int(n_classes)
        if not 1 <= n_classes <= MAX_CLASSES:
            raise L.GdlError(f"LinearProbe: n_classes must be in [1, {MAX_CLASSES}] (Linear({FEAT}, n)), got {n_classes}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.GdlError("LinearProbe: the probe lives on an MI355X (cuda) device; there is no CPU path")
        self.n_classes = n_classes
        self.gen = torch.Generator()
        self.gen.manual_seed(int(seed))
        # nn.init.xavier_normal_: std = sqrt(2 / (fan_in + fan_out))
        w = torch.empty((n_classes, FEAT)).normal_(0.0, math.sqrt(2.0 / (FEAT + n_classes)), generator=self.gen)
        self.weight = w.to(self.device)
        self.bias = torch.zeros(n_classes, device=self.device)
        self.momentum_weight = torch.zeros_like(self.weight)
        self.momentum_bias = torch.zeros_like(self.bias)
        self.epoch = 0
        self._ws = {}

    def _check_bank(self, bank):
        if not isinstance(bank, FeatureBank) or bank.device != self.device:
            raise L.GdlError(f"LinearProbe: a gdl.FeatureBank on {self.device} is expected")

    def fit(self, bank, epochs, batch_size=64, lr=1e-3, momentum=0.9, weight_decay=1e-4, max_norm=40.0, order=None):
        """`epochs` epochs of the fused step on `bank`; returns the epochs' mean losses (a list of floats) after ONE
        synchronisation and one host copy.  order=None: one `torch.randperm(N)` per epoch on the probe's generator, the ragged
        tail dropped (`drop_last=True`); otherwise an integer [epochs, steps, batch_size] table of bank rows, checked on the host.
        lr: a float, or one value per epoch (gdl.multistep_lr)."""
        self._check_bank(bank)
        epochs, B = int(epochs), int(batch_size)
        if epochs < 1:
            raise L.GdlError(f"LinearProbe.fit: epochs must be >= 1, got {epochs}")
        lrs = [float(lr)] * epochs if np.ndim(lr) == 0 else [float(v) for v in lr]
        if len(lrs) != epochs:
            raise L.GdlError(f"LinearProbe.fit: lr must be a float or hold one value per epoch ({epochs}), got {len(lrs)}")
        tab = probe_order(bank.N, B, epochs, self.gen) if order is None else check_order(order, bank.N, epochs, B)
        steps, n = tab.shape[1], self.n_classes
        lib = L.load()
        with torch.cuda.device(self.device):
            tab_d = tab.to(self.device)
            acc = torch.zeros((epochs, 2), dtype=torch.float64, device=self.device)
            ws = self._ws.get(B)
            if ws is None:
                ws = self._ws[B] = torch.zeros(lib.gdl_linprobe_workspace_bytes(B, n), dtype=torch.uint8, device=self.device)
            st = L.cur_stream()
            for e in range(epochs):
                L.call("gdl_linprobe_epoch", L.ptr(bank.features), L.ptr(bank.labels), bank.N, tab_d[e].data_ptr(), steps, B,
                       L.ptr(self.weight), L.ptr(self.bias), L.ptr(self.momentum_weight), L.ptr(self.momentum_bias), n, lrs[e],
                       float(momentum), float(weight_decay), float(max_norm), acc[e].data_ptr(), L.ptr(ws), ws.numel(), st)
            a = acc.cpu().numpy()
        self.epoch += epochs
        return [float(s / c) if c else float("nan") for s, c in a]

    def score(self, bank, chunk=4096, scores=None):
        """(accuracy, counts [2, n] int64: per class the samples seen and the samples right) of arg-max(f W^T + b) over the
        bank; the first maximum wins, as np.argmax.  gdl_head_cls_fwd in chunks + gdl_eval_count, one host copy.
        scores: a gdl.ScoreBank of sets = 1 that every chunk is appended to behind its counters (mAP / top-k / confusion from
        `scores.report()`), refused before the first launch if it does not fit; the return value does not change."""
        self._check_bank(bank)
        n = self.n_classes
        if scores is not None:
            scores.check(n, 1, self.device, bank.N, "LinearProbe.score")
        with torch.cuda.device(self.device):
            cnt = torch.zeros((2, n), dtype=torch.int64, device=self.device)
            out = torch.empty((min(chunk, bank.N), n), device=self.device)
            st = L.cur_stream()
            for o in range(0, bank.N, chunk):
                B = min(chunk, bank.N - o)
                L.call("gdl_head_cls_fwd", bank.features[o:o + B].data_ptr(), L.ptr(self.weight), L.ptr(self.bias), L.ptr(out), B, n,
                       FEAT, st)
                L.call("gdl_eval_count", L.ptr(out), None, None, bank.labels[o:o + B].data_ptr(), B, n, cnt[0].data_ptr(),
                       cnt[1].data_ptr(), None, None, st)
                if scores is not None:
                    scores.append(out[:B], None, None, bank.labels[o:o + B], stream=st)
            c = cnt.cpu().numpy()
        return float(c[1].sum()) / max(float(c[0].sum()), 1.0), c

    def state_dict(self):
        """weight, bias, both momentum buffers (copies), the epoch count and the generator's state: a fit resumed from it is
        bit-equal to the uninterrupted one (given the same order table, or the same generator state with order=None)."""
        return {"weight": self.weight.clone(), "bias": self.bias.clone(), "momentum_weight": self.momentum_weight.clone(),
                "momentum_bias": self.momentum_bias.clone(), "epoch": self.epoch, "generator": self.gen.get_state()}

    def load_state_dict(self, sd):
        n = self.n_classes
        for k, shape in (("weight", (n, FEAT)), ("bias", (n,)), ("momentum_weight", (n, FEAT)), ("momentum_bias", (n,))):
            if tuple(sd[k].shape) != shape:
                raise L.GdlError(f"LinearProbe.load_state_dict: {k} has shape {tuple(sd[k].shape)}, expected {shape}")
        for k in ("weight", "bias", "momentum_weight", "momentum_bias"):
            getattr(self, k).copy_(sd[k].to(self.device, torch.float32))
        self.epoch = int(sd["epoch"])
        if sd.get("generator") is not None:
            self.gen.set_state(sd["generator"])
