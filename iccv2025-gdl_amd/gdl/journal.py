"""The step journal: the reference scripts' per-step log kept on the device (csrc/journal.hip behind gdl_journal_append).

main_dgl.py appends [audio_grad_sum, visual_grad_sum] to a CSV at every step (:132-152), adds the three losses' `.item()` into
its epoch sums (:156-165) and prints them with `torch.abs(out_a).mean()` / `torch.abs(out_v).mean()` every 100 steps (:125-127,
:144-146); main.py adds the two diversity sums (:339-340) and OGM's ratio and coefficients (:308-312).  One launch per step
writes all of them as a row of `len(COLUMNS)` floats into a ring on the device and adds the row to the epoch's float64 sums
beside it; `Journal.fetch()` is the one host copy that brings back the cursor, the sums and the rows.  The runners own one
behind `DGLTrainer(..., journal=capacity)` / `UnimodalTrainer(..., journal=capacity)` and hand it out as `tr.journal()`.
"""
import numpy as np
import torch

from . import _lib as L

# the columns of a row, in order (include/gdl_hip.h: GDL_JOURNAL_COLS of them)
COLUMNS = ("loss_f", "loss_a", "loss_v", "total_norm", "clip_coef", "audio_grad_sum", "visual_grad_sum", "abs_out_a", "abs_out_v",
           "a_diversity", "v_diversity", "score_a", "score_v", "ratio_v", "coeff_a", "coeff_v")
N_ACC = 11          # columns 0 .. 10 have an epoch sum on the device
HEADER_BYTES = 128  # int64 count + 3 reserved, double acc[12]; the rows follow
_ACC_AT = 32


class Journal:
    """A device buffer of gdl_journal_bytes(capacity) and the calls on it.  Appends must be ordered on one stream."""

    def __init__(self, capacity, device):
        capacity = int(capacity)
        nbytes = L.load().gdl_journal_bytes(capacity)
        if nbytes == 0:
            raise L.GdlError(f"gdl.journal.Journal: capacity must be at least 1 row, got {capacity}")
        self.capacity = capacity
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)

    def append(self, losses, stats, out_a=None, out_v=None, n_logits=0, div_a=None, div_v=None, ogm=None, stream=None):
        """One row behind whatever wrote the sources on `stream` (None: the current one).  losses: a device tensor of 3 floats,
        or of 1 (written to all three loss columns); the others: device pointers (int) or None = NaN in their columns."""
        L.call("gdl_journal_append", self.buf.data_ptr(), self.capacity, L.ptr(losses), losses.numel(), stats, out_a, out_v,
               n_logits, div_a, div_v, ogm, L.cur_stream() if stream is None else stream)

    def reset(self):
        """Zeroes the cursor and the sums on the current stream (the rows need no clearing): a new epoch."""
        self.buf[:HEADER_BYTES].zero_()

    def fetch(self):
        """(count, acc, rows): the number of appends since the last reset, the float64 sums of columns 0 .. N_ACC - 1 over all
        of them, and the retained rows -- the newest min(count, capacity) -- in step order as float32 [n, 16].  ONE host copy
        of the whole buffer on the current stream."""
        h = self.buf.cpu().numpy()
        count = int(h[:8].view(np.int64)[0])
        acc = h[_ACC_AT:_ACC_AT + 8 * N_ACC].view(np.float64).copy()
        ring = h[HEADER_BYTES:].view(np.float32).reshape(self.capacity, len(COLUMNS))
        if count <= self.capacity:
            rows = ring[:max(count, 0)].copy()
        else:
            at = count % self.capacity  # the oldest retained row
            rows = np.concatenate([ring[at:], ring[:at]])
        return count, acc, rows
