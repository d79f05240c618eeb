"""Class prototypes for prototypical modal rebalance (PMR, Fan et al., CVPR 2023) on the joint-training runner.

    protos = gdl.Prototypes(n_classes, device, momentum=0.2)
    tr = DGLTrainer(model, lr, mode="joint", prototypes=protos, alpha=1.0, modulation_starts=0, modulation_ends=50)
    for epoch in range(epochs):
        tr.epoch = epoch
        model.eval()                                        # (the banks are eval-mode features: BatchNorm running statistics)
        protos.update(gdl.extract_features(model, "audio", subset), gdl.extract_features(model, "visual", subset))
        model.train()
        for spec, image, label in loader:
            tr.step(spec, image, label)

A prototype is the mean pooled feature of a class over a feature bank -- any subset of the training set the caller chooses (the
published script takes a tenth of it) -- smoothed over the epochs: the first `update` sets P_c = mean_c, every later one
P_c = (1 - momentum) P_c + momentum mean_c.  One launch per bank (gdl_proto_update, csrc/proto.hip): class sums in ascending row
order in float64, rounded to float32 once; nothing is copied to the host and nothing synchronises.  DESIGN.md section 8 states the
arithmetic of the step's prototype term and what is not built (the paper's entropy regulariser, the Swin branch, process groups).
"""
import torch

from . import _lib as L
from .probe import FEAT, MAX_CLASSES, FeatureBank


class Prototypes:
    """`audio` / `visual` [n, 512] float32 (zero before the first `update`), `count` [2, n] int64 (rows per class in the last
    banks), `info` [2, 2] int64 (per modality: classes that had no row, rows whose label was outside [0, n)) -- all on the
    device, written in stream order -- and `updates`, the number of `update` calls so far (host)."""

    def __init__(self, n_classes, device, momentum=0.2):
        if isinstance(n_classes, bool) or not isinstance(n_classes, int) or not 1 <= n_classes <= MAX_CLASSES:
            raise L.GdlError(f"Prototypes: n_classes must be an int in [1, {MAX_CLASSES}], got {n_classes!r}")
        momentum = float(momentum)
        if not 0.0 <= momentum <= 1.0:  # (NaN fails both)
            raise L.GdlError(f"Prototypes: momentum must be in [0, 1], got {momentum}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.GdlError("Prototypes: the prototypes live on an MI355X (cuda) device; there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_classes, self.momentum = n_classes, momentum
        self.protos = torch.zeros((2, n_classes, FEAT), device=self.device)
        self.count = torch.zeros((2, n_classes), dtype=torch.int64, device=self.device)
        self.info = torch.zeros((2, 2), dtype=torch.int64, device=self.device)
        self.updates = 0

    @property
    def audio(self):
        return self.protos[0]

    @property
    def visual(self):
        return self.protos[1]

    @property
    def empty(self):
        """[2] int64 (device): per modality the classes the last banks had no row for -- they kept their prototypes"""
        return self.info[:, 0]

    def _check_bank(self, bank, which):
        if not isinstance(bank, FeatureBank):
            raise L.GdlError(f"Prototypes.update: bank_{which} must be a gdl.FeatureBank, got {type(bank).__name__}")
        if bank.device != self.device:
            raise L.GdlError(f"Prototypes.update: bank_{which} is on {bank.device}, the prototypes on {self.device}")
        if bank.features.shape[1] != FEAT or bank.N < 1:
            raise L.GdlError(f"Prototypes.update: bank_{which} must hold [N >= 1, {FEAT}] features, got {tuple(bank.features.shape)}")
        if bank.modality not in (None, which):
            raise L.GdlError(f"Prototypes.update: bank_{which} holds {bank.modality!r} features")

    def update(self, bank_audio, bank_visual):
        """One gdl_proto_update per bank on the current stream.  The banks are checked on the host for type, device, width and
        modality; the labels stay on the device, so their range is checked THERE: a row whose label is outside [0, n) belongs to
        no class and is counted in `info[:, 1]` -- `check()` raises on it (one synchronisation, when the caller can afford one)."""
        self._check_bank(bank_audio, "audio")
        self._check_bank(bank_visual, "visual")
        with torch.cuda.device(self.device):
            st = L.cur_stream()
            for m, bank in enumerate((bank_audio, bank_visual)):
                L.call("gdl_proto_update", L.ptr(bank.features), L.ptr(bank.labels), bank.N, L.ptr(self.protos[m]), self.n_classes,
                       FEAT, self.momentum, int(self.updates == 0), L.ptr(self.count[m]), L.ptr(self.info[m]), st)
        self.updates += 1

    def check(self):
        """Synchronises; raises if the last banks held a label outside [0, n).  Returns {'empty': [audio, visual]}."""
        info = self.info.cpu().numpy()
        if info[:, 1].any():
            raise L.GdlError(f"Prototypes: the last banks held {int(info[0, 1])} (audio) / {int(info[1, 1])} (visual) rows whose label "
                             f"is outside [0, {self.n_classes})")
        return {"empty": [int(info[0, 0]), int(info[1, 0])]}

    def state_dict(self):
        return {"prototypes": self.protos.clone(), "count": self.count.clone(), "info": self.info.clone(), "updates": self.updates,
                "momentum": self.momentum, "n_classes": self.n_classes}

    def load_state_dict(self, sd):
        if int(sd["n_classes"]) != self.n_classes or tuple(sd["prototypes"].shape) != (2, self.n_classes, FEAT):
            raise L.GdlError(f"Prototypes.load_state_dict: the checkpoint holds {int(sd['n_classes'])} classes "
                             f"{tuple(sd['prototypes'].shape)}, these prototypes {self.n_classes}")
        self.protos.copy_(sd["prototypes"].to(self.device, torch.float32))
        self.count.copy_(sd["count"].to(self.device))
        self.info.copy_(sd["info"].to(self.device))
        self.updates, self.momentum = int(sd["updates"]), float(sd["momentum"])


def prototype_logits(features, prototypes):
    """sim [B, n] = -||features[b] - prototypes[j]|| for a caller's own float32 [B, 512] / [n, 512] device tensors, as the step
    computes it (gdl_proto_ce's `sim` output; the distance is a direct sum of squared differences).  arg-max over j is the
    nearest-prototype classifier."""
    for name, t in (("features", features), ("prototypes", prototypes)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != FEAT or t.dtype != torch.float32 or not t.is_contiguous():
            raise L.GdlError(f"prototype_logits: {name} must be a contiguous float32 [rows, {FEAT}] tensor")
        if t.device.type != "cuda":
            raise L.GdlError("prototype_logits: the tensors must live on an MI355X (cuda) device; there is no CPU path")
    if prototypes.device != features.device:
        raise L.GdlError(f"prototype_logits: features on {features.device}, prototypes on {prototypes.device}")
    B, n = features.shape[0], prototypes.shape[0]
    if B < 1 or not 1 <= n <= MAX_CLASSES:
        raise L.GdlError(f"prototype_logits: B >= 1 rows and 1 <= n <= {MAX_CLASSES} prototypes, got {B} and {n}")
    with torch.cuda.device(features.device):
        sim = torch.empty((B, n), device=features.device)
        labels = torch.zeros(B, dtype=torch.int64, device=features.device)
        u, terms = torch.empty((B, FEAT), device=features.device), torch.empty((2, B), device=features.device)
        L.call("gdl_proto_ce", L.ptr(features), L.ptr(prototypes), L.ptr(labels), L.ptr(u), L.ptr(terms), L.ptr(sim), B, n, FEAT,
               L.cur_stream())
    return sim
