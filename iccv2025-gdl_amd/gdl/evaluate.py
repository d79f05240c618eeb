"""The evaluation report on the device: mAP, top-k and confusion matrices beside valid()'s three accuracies (csrc/evalbank.hip
behind gdl_eval_bank_append / gdl_eval_bank_ap).

The reference's valid() returns (acc, acc_a, acc_v); the tables this work is compared in also give mAP (OGM-GE, PMR, MLA,
MMPareto on Kinetics-Sounds and VGGSound), top-5 (309 / 400 classes) and start every per-class analysis of modality imbalance
from the confusion matrices of the audio-only and visual-only logit sets.  This is not a port of a reference script: like the
linear probe it goes beyond the reference because the papers report the number.  A `ScoreBank` is one device buffer; every batch
is one launch behind `gdl_eval_count` on the same stream (softmax scores stored class-major, the label's rank, the confusion
entry), `report()` is one launch pair for the average precisions, one synchronisation and ONE host copy.

    bank = gdl.ScoreBank(n_classes, capacity=len(val_set), sets=3, device="cuda:0")
    acc, acc_a, acc_v = trainer.valid(batches, bank=bank)      # unchanged return value
    r = bank.report(ks=(1, 5))                                 # r["mAP"], r["topk"][5], r["confusion"][1], ...
"""
import numpy as np
import torch

from . import _lib as L

MAX_CLASSES = 512  # HB_MAXN of csrc/head_body.h
SET_NAMES = ("fused", "audio", "visual")


def _align16(v):
    return (v + 15) // 16 * 16


class ScoreBank:
    """A device buffer of gdl_eval_bank_bytes(n_classes, capacity, sets) and the calls on it (the layout: include/gdl_hip.h).
    sets = 3: the fused, audio and visual logit sets of a DGL / multi-task model; sets = 1: the one set of a jointly trained or
    unimodal model, or of a linear probe.  `N` is the number of rows appended since the last reset -- the only host-side state.
    Calls on one bank must be ordered on one stream."""

    def __init__(self, n_classes, capacity, sets=3, device="cuda"):
        n_classes, capacity, sets = int(n_classes), int(capacity), int(sets)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.GdlError("ScoreBank: the bank lives on an MI355X (cuda) device; there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        lib = L.load()
        nbytes = lib.gdl_eval_bank_bytes(n_classes, capacity, sets)
        if nbytes == 0:
            raise L.GdlError(f"ScoreBank: n_classes must be in [1, {MAX_CLASSES}], capacity in [1, 2^31) and sets 1 or 3; got "
                             f"n_classes = {n_classes}, capacity = {capacity}, sets = {sets}")
        self.n_classes, self.capacity, self.sets = n_classes, capacity, sets
        self._reset_bytes = lib.gdl_eval_bank_reset_bytes(n_classes, sets)
        self._map_at = self._reset_bytes + 8 * sets * n_classes
        self._labels_at = _align16(self._map_at + 32)
        self._probs_at = self._labels_at + _align16(4 * capacity)
        assert self._probs_at + 4 * sets * n_classes * capacity == nbytes, "ScoreBank: the layout of include/gdl_hip.h has moved"
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.N = 0

    def check(self, n_classes, sets, device, rows, who="ScoreBank"):
        """Refuses, on the host and before any launch, a bank of another class count, set count or device, or with fewer than
        `rows` free rows."""
        if self.n_classes != n_classes or self.sets != sets:
            raise L.GdlError(f"{who}: a ScoreBank of n_classes = {n_classes}, sets = {sets} is expected, got n_classes = "
                             f"{self.n_classes}, sets = {self.sets}")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device != self.device:
            raise L.GdlError(f"{who}: the ScoreBank is on {self.device}, the logits on {device}")
        if self.N + rows > self.capacity:
            raise L.GdlError(f"{who}: {rows} rows behind the {self.N} already held do not fit a capacity of {self.capacity}")

    def append(self, out, out_a=None, out_v=None, label=None, stream=None):
        """One launch behind whatever wrote the logits on `stream` (None: the current one): out (and, for sets = 3, out_a and
        out_v) float32 [B, n_classes], label int64 [B], all contiguous on the bank's device."""
        if label is None or out is None:
            raise L.GdlError("ScoreBank.append: out and label are required")
        given = [t for t in (out, out_a, out_v) if t is not None]
        if len(given) != self.sets:
            raise L.GdlError(f"ScoreBank.append: a bank of sets = {self.sets} takes {self.sets} logit set(s), got {len(given)}")
        B = out.shape[0] if out.dim() == 2 else -1
        for t in given:
            if t.dtype != torch.float32 or tuple(t.shape) != (B, self.n_classes) or not t.is_contiguous():
                raise L.GdlError(f"ScoreBank.append: logits must be contiguous float32 [B, {self.n_classes}], got {t.dtype} "
                                 f"{tuple(t.shape)}")
        if label.dtype != torch.int64 or tuple(label.shape) != (B,) or not label.is_contiguous():
            raise L.GdlError(f"ScoreBank.append: label must be a contiguous int64 [B = {B}] tensor")
        for t in given + [label]:
            if t.device != self.device:
                raise L.GdlError(f"ScoreBank.append: the bank is on {self.device}, a tensor on {t.device}")
        self.check(self.n_classes, self.sets, self.device, B, "ScoreBank.append")
        with torch.cuda.device(self.device):
            L.call("gdl_eval_bank_append", self.buf.data_ptr(), self.buf.numel(), self.n_classes, self.capacity, self.sets,
                   L.ptr(out), L.ptr(out_a), L.ptr(out_v), L.ptr(label), B, self.N, L.cur_stream() if stream is None else stream)
        self.N += B

    def reset(self):
        """Zeroes the counters on the current stream (gdl_eval_bank_reset_bytes; scores and labels need no clearing) and the
        row count: a new report."""
        self.buf[:self._reset_bytes].zero_()
        self.N = 0

    def report(self, ks=(1, 5)):
        """The report over the N rows appended since the last reset: gdl_eval_bank_ap on the current stream, then ONE host copy
        (which synchronises).  Index s runs over the bank's sets (SET_NAMES: fused, audio, visual).
          N              rows appended, skipped ones included
          skipped        samples whose label lies outside [0, n): they count nowhere else
          nonfinite      [sets] rows holding a NaN / inf logit: left out of that set's confusion, top-k and ap
          num            [n] int64, samples per class
          confusion      [sets, n, n] int64, row = label, column = prediction (first maximum, as valid())
          rank_hist      [sets, n] int64, [s][r] = counted rows whose label has rank r (r logits beat it; ties count for the
                         lower class)
          per_class_acc  [sets, n] = diagonal / row sum of confusion; NaN for a class no row of which was counted
          topk           {k: [sets]}: the share of counted rows whose label is among the k largest logits (ties broken towards
                         the lower class, so top-1 is valid()'s accuracy whenever no row was left out)
          ap             [sets, n] float64 average precision of the float32 softmax scores, scikit-learn's
                         average_precision_score (step-wise, ties grouped); NaN for a class without a positive, where
                         scikit-learn returns 0.0 with a warning
          mAP            [sets] float64 mean of the non-NaN ap in class order"""
        n, S = self.n_classes, self.sets
        ks = tuple(int(k) for k in ks)
        if any(k < 1 for k in ks):
            raise L.GdlError(f"ScoreBank.report: every k must be at least 1, got {ks}")
        with torch.cuda.device(self.device):
            L.call("gdl_eval_bank_ap", self.buf.data_ptr(), self.buf.numel(), n, self.capacity, S, self.N, L.cur_stream())
            h = self.buf[:self._map_at + 8 * S].cpu().numpy()
        i64 = h[:self._reset_bytes].view(np.int64)
        num = i64[4:4 + n].copy()
        hist = i64[4 + n:4 + n + S * n].reshape(S, n)
        conf = i64[4 + n + S * n:].reshape(S, n, n).copy()
        f64 = h[self._reset_bytes:].view(np.float64)
        counted = hist.sum(axis=1).astype(np.float64)
        rows = conf.sum(axis=2).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            pca = np.where(rows > 0, conf.diagonal(axis1=1, axis2=2) / rows, np.nan)
            topk = {k: [float(hist[s, :k].sum()) / counted[s] if counted[s] else float("nan") for s in range(S)] for k in ks}
        return {"N": self.N, "skipped": int(i64[0]), "nonfinite": [int(v) for v in i64[1:1 + S]], "num": num, "confusion": conf,
                "rank_hist": hist.copy(), "per_class_acc": pca, "topk": topk, "ap": f64[:S * n].reshape(S, n).copy(), "mAP": f64[S * n:S * n + S].copy()}

    def scores(self):
        """(labels int32 [N], probs float32 [sets, n, N]) as stored -- a second host copy, for inspection: -1 marks a skipped
        sample, NaN a row left out of a set."""
        n, S, cap = self.n_classes, self.sets, self.capacity
        lab = self.buf[self._labels_at:self._labels_at + 4 * cap].cpu().numpy().view(np.int32)[:self.N].copy()
        pr = self.buf[self._probs_at:].cpu().numpy().view(np.float32).reshape(S, n, cap)[:, :, :self.N].copy()
        return lab, pr
