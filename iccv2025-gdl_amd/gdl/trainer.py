"""Native DGL training step: the whole body of /root/reference/main_dgl.py:97-154 as one
sequence of gfx950 kernels on two HIP streams (+ a side stream for the visual weight gradients), without an autograd tape.

Per step (all asynchronous, nothing is read back unless `read()` is called).  Default form for the concat / sum DGL heads
(the Swin composition's 512 + 768 concat head included) without a process group ("early backward", bit-identical to the
junction form below):
  stream V: visual forward -> gdl_head_uni_dfeat (alpha * dCE(v_out)/d feature) -> visual backward
  stream A: audio  forward -> gdl_head_uni_dfeat (alpha * dCE(a_out)/d feature) -> audio  backward
            -> fusion head forward (all three logit sets), 3x cross-entropy, gradient of fc_out from loss_f alone
  then on A: fused grad statistics (total norm -> clip coefficient, per-encoder sum mean|g|)  (main_dgl.py:129-143)
             fused clip + SGD(momentum, weight decay) over the flat parameter arena            (:154)
             (or AdamW / Adagrad: `optimizer`, the script's --optimizer switch, :248-259)
Junction form (other heads, the joint step -- mode="joint": ONE cross-entropy on the fused logits whose gradient flows through
the head into both encoders, BASELINE config 1, for all four heads -- and -- until a multi-GPU run has validated the early form's collective order --
every data-parallel run):
  audio encoder forward  (stream A)  ||  visual encoder forward (stream V)
  fusion head forward, 3x cross-entropy, head backward with the DGL truncation   (stream A)
      - encoders receive only alpha * d(CE(a_out) + CE(v_out))      (main_dgl.py:108-110)
      - fc_out receives only d CE(out) on detached features          (:114-122)
      - fc_auxi never receives a gradient and is skipped by SGD      
  audio encoder backward (stream A)  ||  visual encoder backward (stream V)
      [+ per-bucket RCCL all-reduce as soon as a bucket is final]
  grad statistics, clip + SGD as above
Joint step with modulation="OGM" / "OGM_GE" (main.py:286-330; concat and sum heads): gdl_head_uni_scores behind the head forward
(the unimodal scores, on the device), and gdl_optim_modulate between the statistics and the update -- the convolution weight
gradients of both encoders become (g k) c [+ sigma z] in the arena, the update takes the arena as it stands.
Joint step with `prototypes=` (prototypical modal rebalance, gdl.prototypes; all four heads): gdl_proto_ce behind each encoder's
forward on its own stream, gdl_proto_apply behind the head's feature gradients in front of the junction event -- the feature
gradient of the modality that is behind gains alpha * d lossp / d feature, nothing else changes.

DGL ablations (mode="dgl"; `detach_fused`, `drop_head_uni`): DGL is two truncations of one three-loss step -- the fused logits are
detached (main_dgl.py:100-108, the .detach() inside every *_DGL head) and the unimodal losses' gradients in the fusion module are
dropped (:114-122).  drop_head_uni=False keeps the latter (the head kernels' uni_in_dw = 1; every form above still applies).
detach_fused=False (concat / sum head, ResNet18 encoders) lets loss_f reach the encoders: an encoder's feature gradient then
needs both encoders' features, so the step is the junction form with ONE launch at the junction,
  both forwards -> gdl_head_mtl_ce (three logit sets, three losses, their gradients, dfa / dfv) -> event -> both backward chains,
and the head's parameter gradients behind the junction on the audio stream.  Both off = the multi-task baseline
loss_f + gamma (loss_a + loss_v) of main.py:177 under plain autograd (alpha = the scripts' --gamma).

MMPareto integration on the multi-task step (`pareto=True`): the junction computes the unimodal losses' feature
gradients (gdl_head_mtl_ce with fused_reaches = 0) and the fused loss' (one gdl_head_*_bwd from g_f) separately; each encoder's
stream then carries two backwards of its one forward -- into the gradient arena and into a second arena -- and
gdl_pareto_integrate, which leaves the integrated gradient in the arena.  The tail is the same.

ArenaTrainer below is what such a runner is before it knows its model (the flat arenas, the optimizer state and its checkpoint,
the chain streams, the statistics + clip + update tail); DGLTrainer is the step above on it, gdl.unimodal.UnimodalTrainer the
one-encoder step.

The result is numerically the reference's two-phase backward: SURVEY section 0 shows the
single-pass form is bit-identical in exact arithmetic, and tests/test_step_gpu.py checks it
against golden vectors of the reference.
"""
import ctypes
import os

import torch

from . import _lib as L
from .encoder import EncoderEngine


class _SwinAdapter:
    """gdl.swin.SwinEngine behind the EncoderEngine calls the trainer makes (features averaged over the T frames of a
    sample; no BatchNorm state; phase 1 = upstream gradient + final norm + last stage, phase 2 = the rest)."""

    def __init__(self, cfg, dtype, B, T, device, net=None):
        from .swin import SwinEngine

        self.eng = SwinEngine(cfg, dtype, B, T, device)
        self.net = net  # the mirror module: drop_path_rate, drop_scales_override / last_drop_scales (stochastic depth)

    def set_params(self, params):
        self.eng.set_params(params)

    def forward(self, x, training, feat_out=None):
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise L.GdlError("DGLTrainer: frames must be a contiguous float32 [B, 3, T, H, W] tensor")
        drop = None
        if training and self.net is not None and self.net.drop_path_rate > 0:  # a training step draws the DropPath masks
            import sys

            drop_path_scales = sys.modules[type(self.net).__module__].drop_path_scales  # (models.swin_transformer, as imported by the caller)
            drop = self.net.drop_scales_override if self.net.drop_scales_override is not None else \
                drop_path_scales(self.eng.cfg, self.net.drop_path_rate, self.eng.N, self.eng.device)
            self.net.last_drop_scales = drop
        return self.eng.forward(x, pool_frames=True, out=feat_out, drop_scales=drop)

    def backward(self, grads, dfeat=None, phase=0):
        if phase != 2:
            self._dfeat = dfeat
        self.eng.backward(self._dfeat, list(grads), phase=phase)


# The optimizers of main_dgl.py's `--optimizer` switch (:248-259), keyed by the script's own strings, and what it builds for
# each: SGD(momentum=0.9, weight_decay=1e-4), Adagrad(lr) and AdamW(lr, betas=(0.9, 0.999)) -- the latter two with torch's
# defaults for everything else.  These are the reference's values, not options; `weight_decay` may be overridden.
OPTIMIZERS = ("sgd", "Adam", "AdaGrad")
DEFAULT_WEIGHT_DECAY = {"sgd": 1e-4, "Adam": 1e-2, "AdaGrad": 0.0}
ADAM_BETAS = (0.9, 0.999)
ADAM_EPS = 1e-8
ADAGRAD_EPS = 1e-10
ADAGRAD_INITIAL_ACCUMULATOR = 0.0
# main.py's `--modulation` (:286-330): "Normal" = none; "OGM" = the encoder whose unimodal score leads has its convolution weight
# gradients scaled by 1 - tanh(alpha * ratio); "OGM_GE" = the same plus N(0, std(g) + 1e-8) noise on both encoders' (CVPR 2022)
MODULATIONS = ("Normal", "OGM", "OGM_GE")

_CHAIN_STREAMS = {}


def _chain_streams(device):
    """(audio-chain stream, visual-chain stream) of `device`, created once per process"""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _CHAIN_STREAMS:
        _CHAIN_STREAMS[key] = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
    return _CHAIN_STREAMS[key]


class ArenaTrainer:
    """What a native step runner is before it knows its model: the trained tensors laid out in one flat parameter arena and one
    gradient arena (the modules alias the former), the chosen optimizer's state arenas and their checkpoint, the library's
    optimizer descriptor, the two chain streams, and the tail of every step -- gradient statistics, clip, update.  A subclass
    supplies the (name, parameter) list with its optimizer groups (0 = head, 1 = audio encoder, 2 = visual encoder: the
    statistics' `audio_grad_sum` / `visual_grad_sum`) and the body of the step in front of `_finish_step`."""

    _script = "main_dgl.py"  # the reference script whose --optimizer the class takes

    @classmethod
    def _check_optimizer(cls, optimizer):
        """(subclasses call this before they touch the model: a wrong name is refused first)"""
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"{cls.__name__}: optimizer must be one of {OPTIMIZERS} ({cls._script} --optimizer), got {optimizer!r}")

    def __init__(self, named, group, device, optimizer, lr, momentum, weight_decay, max_norm):
        """named: [(name, parameter)] in arena order; group: the optimizer group of each; optimizer: the scripts'
        `args.optimizer` -- "sgd" (momentum, weight decay), "Adam" (AdamW) or "AdaGrad"; weight_decay None = the reference's value
        for that optimizer (DEFAULT_WEIGHT_DECAY); `momentum` applies to "sgd" only."""
        self._check_optimizer(optimizer)
        self.optimizer = optimizer
        if weight_decay is None:
            weight_decay = DEFAULT_WEIGHT_DECAY[optimizer]
        self.lib = L.load()
        self.device = device
        self.lr, self.mu, self.wd, self.max_norm = float(lr), float(momentum), float(weight_decay), float(max_norm)
        self.names = [n for n, _ in named]
        offs, o = [0], 0
        for _, p in named:
            o += p.numel()
            offs.append(o)
        self.offsets = offs
        self.total = o
        self.params = torch.empty(o, device=self.device)
        self.grads = torch.zeros(o, device=self.device)
        # optimizer state arenas (the parameter arena's layout), only those of the chosen optimizer
        self.momentum = self.exp_avg = self.exp_avg_sq = self.state_sum = None
        if optimizer == "sgd":
            self.momentum = torch.zeros(o, device=self.device)
        elif optimizer == "Adam":
            self.exp_avg = torch.zeros(o, device=self.device)
            self.exp_avg_sq = torch.zeros(o, device=self.device)
        else:
            self.state_sum = torch.full((o,), ADAGRAD_INITIAL_ACCUMULATOR, device=self.device)
        self.pviews, self.gviews = [], []
        for i, (_, p) in enumerate(named):
            v = self.params[offs[i]:offs[i + 1]].view(p.shape)
            v.copy_(p.data)
            p.data = v  # the module now aliases the arena: state_dict / eval see the trained weights
            self.pviews.append(v)
            self.gviews.append(self.grads[offs[i]:offs[i + 1]].view(p.shape))
        self._create_descriptors(offs, group)
        # The two chain streams are shared by every trainer of a process on this device: torch hands out a NEW pool stream per
        # torch.cuda.Stream() call and never retires one, and once more distinct streams have carried work than the runtime has
        # hardware queues (four), two chains can end up time-slicing one queue -- the third trainer built in a process ran its step
        # 15 % slower than the same trainer in a fresh process (bench.py's `extra_workloads.ks`: 7.33 vs 6.36 ms, round 4).
        self.s_a, self.s_v = _chain_streams(self.device)
        # a data-parallel subclass sets both: `_finish_step` waits for the reducer and scales by 1 / world, `close` releases it
        self.reducer = None
        self.world = 1
        self.steps = 0
        self.phase_events = None  # set to [] to record (name, event) marks on the main stream per step
        # measuring tap (bench.py): a [n, 2] device tensor + a position; while the position is not None every step copies its
        # (total norm, clip coefficient) into the next row, device to device on the step's stream
        self.stats_log = None
        self.stats_log_pos = None
        # gradient modulation (a subclass calls `_setup_modulation`): None = the step launches none of its kernels
        self._mod = None
        self._mod_now = False
        # the feature-diversity monitor (a subclass calls `_setup_diversity`): () = nothing allocated, nothing launched
        self._div_keys = ()
        # the step journal (a subclass calls `_setup_journal`): None = nothing allocated, nothing launched
        self._journal = None

    def _descriptor(self, offs, group):
        """(descriptor, workspace bytes, workspace, statistics) of the library's optimizer over the segments `offs` (len(group) + 1
        element offsets from the pointers its calls are given) with the optimizer groups `group`"""
        h = ctypes.c_void_p()
        so = (ctypes.c_int64 * len(offs))(*offs)
        sg = (ctypes.c_int32 * len(group))(*group)
        L.call("gdl_optim_create", ctypes.byref(h), so, sg, len(group))
        nb = self.lib.gdl_optim_workspace_bytes(h)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=self.device)
        # (explicit: a caching allocator may hand out a block at the address of an earlier trainer's workspace)
        L.call("gdl_optim_bind_workspace", h, L.ptr(ws), nb, L.cur_stream())
        return h, nb, ws, torch.zeros(self.lib.gdl_optim_stats_len(h), device=self.device)

    def _create_descriptors(self, offs, group):
        """One descriptor over the whole arena; a runner whose steps update sub-ranges of it builds its own instead."""
        self.opt, self.opt_ws_bytes, self.opt_ws, self.stats = self._descriptor(offs, group)

    def _setup_modulation(self, marks, noise, alpha, seed):
        """OGM / OGM-GE over the gradient arena: marks[i] = 0 (untouched), 1 (audio) or 2 (visual) per arena tensor; `noise` =
        the GE term.  The subclass leaves {score_a, score_v} in `self.mod_scores` before `_finish_step` of a step it has set
        `self._mod_now` for."""
        lib = self.lib
        nb = lib.gdl_optim_modulate_workspace_bytes(self.opt)
        self.mod_ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=self.device)
        self.mod_stats = torch.zeros(lib.gdl_optim_modulate_stats_len(self.opt), device=self.device)
        self.mod_scores = torch.zeros(2, device=self.device)
        L.call("gdl_optim_modulate_bind", self.opt, (ctypes.c_int32 * len(marks))(*marks), L.ptr(self.mod_ws), nb, L.cur_stream())
        self._mod = (int(bool(noise)), float(alpha), int(seed))

    @classmethod
    def _check_modulation(cls, modulation):
        """(like `_check_optimizer`: before the model is touched)"""
        if modulation not in MODULATIONS:
            raise ValueError(f"{cls.__name__}: modulation must be one of {MODULATIONS} (main.py --modulation), got {modulation!r}")

    def _setup_diversity(self, keys):
        """main.py's per-step feature-diversity monitor (:77-89, :183-184) for the encoders named by `keys` ("a_diversity" /
        "v_diversity"): `div[i]` = the last step's value, `div_acc[i]` = (sum, count) since the last `epoch_diversity` reset --
        both written by the kernel in stream order.  Not part of `state_dict()`: the script restarts them every epoch."""
        self._div_keys = tuple(keys)
        self.div = torch.zeros(len(keys), device=self.device)
        self.div_acc = torch.zeros((len(keys), 2), device=self.device)

    def _diversity(self, eng, i):
        """gdl_encoder_feature_diversity behind `eng`'s training forward, on the current (= that forward's) stream"""
        if self._div_keys:
            eng.feature_diversity(out=self.div[i:i + 1], accum=self.div_acc[i])

    def epoch_diversity(self, reset=True):
        """{a_diversity, v_diversity} (the encoders this runner has): the means of the per-step values since the last reset, as
        main.py:356 divides its running sums by the number of steps -- one host copy for the whole epoch.  NaN before any step.
        reset: start a new epoch.  With a process group the values are the local rank's."""
        if not self._div_keys:
            raise L.GdlError(f"{type(self).__name__}.epoch_diversity: the monitor is off (diversity=False)")
        acc = self.div_acc.cpu().numpy().astype("float64")
        if reset:
            self.div_acc.zero_()
        return {k: (float(a[0] / a[1]) if a[1] > 0 else float("nan")) for k, a in zip(self._div_keys, acc)}

    def _read_diversity(self, r):
        """(read(), behind its synchronisation) the last step's values under their keys; nothing when the monitor is off"""
        if self._div_keys:
            r.update(zip(self._div_keys, (float(v) for v in self.div.cpu().numpy())))
        return r

    @classmethod
    def _check_journal(cls, journal):
        """(like `_check_optimizer`: before the model is touched) the capacity in steps, 0 = off"""
        if isinstance(journal, bool) or not isinstance(journal, int) or journal < 0:
            raise ValueError(f"{cls.__name__}: journal must be a capacity in steps (an int >= 0, 0 = off), got {journal!r}")
        return journal

    def _setup_journal(self, capacity, logits):
        """The scripts' per-step log on the device (gdl.journal, csrc/journal.hip): a ring of `capacity` rows, the epoch's sums
        and the cursor in one device buffer; `_finish_step` appends a row per step.  0 = off.  logits: whether this runner has
        unimodal logits (`_journal_logits`) for the abs_out_a / abs_out_v columns.  Not part of `state_dict()`: the script
        restarts its sums every epoch."""
        self._journal_has_logits = bool(logits)
        if capacity:
            from .journal import Journal

            self._journal = Journal(capacity, self.device)

    def _journal_logits(self):
        """(a subclass with unimodal logits overrides it) the tensors behind the abs_out_a / abs_out_v columns, or None"""
        return None, None

    def _journal_append(self, st):
        """One row behind the update on the step's main stream `st`: every source is final there -- the losses, the logits and
        `mod_stats` were written on it, the statistics just before, and `_finish_step` has joined both chains (the diversity
        values).  The call has the same arguments at every step but for the OGM pointer, which follows `_mod_now`."""
        out_a, out_v = self._journal_logits()
        n_logits = 0 if out_a is None and out_v is None else (out_a if out_a is not None else out_v).numel()
        div = {k: self.div.data_ptr() + 4 * i for i, k in enumerate(self._div_keys)}
        ogm = L.ptr(self.mod_stats) if self._mod is not None and self._mod_now else None
        self._journal.append(self.losses, L.ptr(self.stats), L.ptr(out_a), L.ptr(out_v), n_logits, div.get("a_diversity"),
                             div.get("v_diversity"), ogm, st)

    def journal(self, reset=True):
        """The step journal since the last reset -- one synchronisation and ONE host copy for what the scripts fetch value by
        value at every step.  Returns a dict:
          columns     gdl.journal.COLUMNS, the 16 names
          rows        float32 [n, 16], the retained rows (the newest `journal` of them) in step order; a column with no source
                      in this configuration -- or, for the OGM columns, at a step that was not modulated -- holds NaN
          first_step  the 0-based count of steps this trainer had taken before the step of rows[0] (`self.steps` then)
          count       rows appended since the last reset
          dropped     max(0, count - capacity): rows the ring has overwritten
          means       {name: sum / count} in float64 for the columns among loss_f .. v_diversity that this trainer feeds, from
                      float64 sums the device adds to in step order (the script's `_loss += x.item()`, then `/ len(dataloader)`):
                      over ALL `count` steps, whether or not the ring overflowed; NaN when count is 0
        reset: start a new epoch -- the cursor and the sums are zeroed, ordered on the stream.  main_dgl.py's CSV rows are
        rows[:, 5:7], its epoch line means["loss_f"], means["loss_a"], means["loss_v"].  With a process group the losses and
        logits are the local rank's, the gradient statistics those of the reduced gradient."""
        if self._journal is None:
            raise L.GdlError(f"{type(self).__name__}.journal: the journal is off (journal=0)")
        from .journal import COLUMNS, N_ACC

        torch.cuda.synchronize(self.device)
        count, acc, rows = self._journal.fetch()
        if reset:
            self._journal.reset()
        fed = set(COLUMNS[:7]) | set(self._div_keys) | ({"abs_out_a", "abs_out_v"} if self._journal_has_logits else set())
        means = {k: (float(acc[i] / count) if count > 0 else float("nan")) for i, k in enumerate(COLUMNS[:N_ACC]) if k in fed}
        return {"columns": COLUMNS, "rows": rows, "first_step": self.steps - rows.shape[0], "count": count,
                "dropped": max(0, count - self._journal.capacity), "means": means}

    def _opt_state(self):
        """{name: arena} of the chosen optimizer's state: momentum (sgd), exp_avg + exp_avg_sq (Adam), state_sum (AdaGrad)."""
        names = {"sgd": ("momentum",), "Adam": ("exp_avg", "exp_avg_sq"), "AdaGrad": ("state_sum",)}[self.optimizer]
        return {n: getattr(self, n) for n in names}

    def state_dict(self):
        """Optimizer-side state a reference checkpoint keeps besides model.state_dict() (optimizer.state_dict() /
        scheduler, main_dgl.py:372): the optimizer's kind and state arenas, learning rate, step count (which the Adam bias
        corrections count from)."""
        sd = {"optimizer": self.optimizer, **{k: v.detach().clone() for k, v in self._opt_state().items()}, "lr": self.lr,
              "steps": self.steps, "names": list(self.names), "offsets": list(self.offsets), "mu": self.mu,
              "weight_decay": self.wd}
        if getattr(self, "pe", False):  # the probabilistic-embedding branch: `steps` above and this seed key its noise
            sd.update(pe=True, pe_beta=self.beta, pe_seed=self.seed)
        return sd

    def load_state_dict(self, sd):
        who = type(self).__name__
        if bool(sd.get("pe", False)) != bool(getattr(self, "pe", False)):
            raise L.GdlError(f"{who}.load_state_dict: the checkpoint was trained " + ("with" if sd.get("pe", False) else "without") +
                             " the probabilistic-embedding branch, this trainer runs " + ("without" if sd.get("pe", False) else "with") + " it")
        if list(sd["offsets"]) != list(self.offsets) or list(sd["names"]) != list(self.names):
            raise L.GdlError(f"{who}.load_state_dict: the checkpoint's parameter layout differs from this model's")
        kind = sd.get("optimizer", "sgd")  # (checkpoints written before the optimizer switch are SGD's)
        if kind != self.optimizer:
            raise L.GdlError(f"{who}.load_state_dict: the checkpoint holds {kind!r} state, this trainer runs {self.optimizer!r}")
        for k, v in self._opt_state().items():
            v.copy_(sd[k].to(self.device))
        self.lr, self.steps = float(sd["lr"]), int(sd["steps"])
        if getattr(self, "pe", False):  # the noise continues the checkpoint's stream: its key, and the step count loaded above
            self.seed = int(sd.get("pe_seed", self.seed))

    def close(self):
        """Releases what the trainer owns outside PyTorch's allocator: the optimizer descriptor and, for
        comm_backend="abi", the RCCL communicator (ncclCommDestroy).  Idempotent; also run by __del__."""
        if getattr(self, "reducer", None) is not None:
            self.reducer.close()
        if getattr(self, "opt", None):
            self.lib.gdl_optim_destroy(self.opt)
            self.opt = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_label(self, label):
        """The loss kernels index logits by label: require the reference's dtype and shape (a class index outside
        [0, n) raises a device assert in the reference; here the loss kernel skips the sample and poisons the loss)."""
        if label.dtype != torch.int64 or label.dim() != 1 or label.shape[0] != self.B or label.device != self.device:
            raise L.GdlError(f"{type(self).__name__}: label must be an int64 [B={self.B}] tensor on {self.device}, got "
                             f"{label.dtype} {tuple(label.shape)} on {label.device}")

    def _finish_step(self, main, st):
        """Joins the chains (and the collectives), then gradient statistics + clip + the optimizer's update on `main`."""
        red = self.reducer
        main.wait_stream(self.s_a)
        main.wait_stream(self.s_v)
        if red is not None:
            red.wait_all()
        self._mark(main, "bwd_done")
        gs = 1.0 / self.world
        L.call("gdl_optim_grad_stats", self.opt, L.ptr(self.grads), self.max_norm, gs, L.ptr(self.stats),
               L.ptr(self.opt_ws), self.opt_ws_bytes, st)
        stats = L.ptr(self.stats)
        if self._mod is not None and self._mod_now:
            # main.py:286-330, between the clip and optimizer.step(): the clipped and modulated gradient is written to the arena,
            # the update then takes it as it stands (stats = NULL, grad_scale = 1); the noise counter is the step count
            noise, alpha, seed = self._mod
            L.call("gdl_optim_modulate", self.opt, L.ptr(self.grads), stats, gs, L.ptr(self.mod_scores), alpha, noise, seed,
                   self.steps, L.ptr(self.mod_stats), L.ptr(self.opt_ws), L.ptr(self.mod_ws), st)
            stats, gs = None, 1.0
        if self.optimizer == "sgd":
            L.call("gdl_optim_sgd_step", self.opt, L.ptr(self.params), L.ptr(self.grads), L.ptr(self.momentum),
                   stats, gs, self.lr, self.mu, self.wd, st)
        elif self.optimizer == "Adam":
            L.call("gdl_optim_adamw_step", self.opt, L.ptr(self.params), L.ptr(self.grads), L.ptr(self.exp_avg),
                   L.ptr(self.exp_avg_sq), stats, gs, self.lr, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, self.wd,
                   self.steps + 1, st)
        else:
            L.call("gdl_optim_adagrad_step", self.opt, L.ptr(self.params), L.ptr(self.grads), L.ptr(self.state_sum),
                   stats, gs, self.lr, ADAGRAD_EPS, self.wd, self.steps + 1, st)
        if self._journal is not None:
            self._journal_append(st)
        self._mark(main, "end")
        if self.stats_log is not None and self.stats_log_pos is not None and self.stats_log_pos < self.stats_log.shape[0]:
            self.stats_log[self.stats_log_pos].copy_(self.stats[:2], non_blocking=True)
            self.stats_log_pos += 1
        self.steps += 1

    def _mark(self, stream, name):
        if self.phase_events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(stream)
            self.phase_events.append((name, e))

    def _read_stats(self, engines):
        """The part of read() every runner shares: synchronises, returns the step's gradient statistics, and raises if a
        BatchNorm layer of one of `engines` overflowed."""
        torch.cuda.synchronize(self.device)
        s = self.stats.cpu().numpy()
        nseg = len(self.names)
        # a diverged BatchNorm (statistics beyond the fixed-point headroom, csrc/bnacc.h) must be as loud as the reference's
        # inf / NaN: ReLU turns the NaN statistics' outputs into zeros, so the logits alone may look sane
        bad = sum(e.bn_overflow() for e in engines if e is not None and hasattr(e, "bn_overflow"))
        if bad:
            raise FloatingPointError(f"gdl: the statistics of {bad} BatchNorm layer(s) overflowed in the last training forward "
                                     "(activations of mean magnitude beyond 8192: the run has diverged)")
        return {"total_norm": float(s[0]), "clip_coef": float(s[1]), "audio_grad_sum": float(s[2]),
                "visual_grad_sum": float(s[3]), "grad_norm": dict(zip(self.names, s[4:4 + nseg].tolist())),
                "grad_absmean": dict(zip(self.names, s[4 + nseg:4 + 2 * nseg].tolist()))}

    def grad(self, name):
        return self.gviews[self.names.index(name)]


class DGLTrainer(ArenaTrainer):
    def __init__(self, model, lr, alpha=4.0, momentum=0.9, weight_decay=None, max_norm=40.0, mode="dgl", dtype=None,
                 process_group=None, comm_backend="torch", visual_side_stream=None, early_backward=None, optimizer="sgd",
                 modulation="Normal", modulation_starts=0, modulation_ends=50, seed=0, detach_fused=True, drop_head_uni=True,
                 diversity=False, journal=0, prototypes=None, beta=0.0, pareto=False, pareto_scale=1.0):
        """comm_backend: "torch" -- torch.distributed all_reduce on `process_group` (nccl = RCCL); "abi" -- the library's own
        RCCL communicator (gdl_comm_*), bootstrapped through `process_group`.
        optimizer: main_dgl.py's `args.optimizer` -- "sgd" (momentum, weight decay), "Adam" (AdamW) or "AdaGrad"; weight_decay
        None = the reference's value for that optimizer (DEFAULT_WEIGHT_DECAY); `momentum` applies to "sgd" only.
        modulation: main.py's `--modulation` for the joint step (mode="joint", concat or sum head, no process group): "Normal",
        "OGM" or "OGM_GE" (MODULATIONS); `alpha` is then main.py's `--alpha` (its scripts use 0.8), the modulation runs while
        modulation_starts <= self.epoch <= modulation_ends (the caller sets `epoch`), and `seed` keys OGM_GE's noise, a function
        of (seed, step count, arena position) alone.
        detach_fused, drop_head_uni: the two gradient truncations DGL is made of (mode="dgl"; the defaults are DGL itself).
        drop_head_uni=False: the fusion head also learns from the unimodal losses -- the unmodified AVClassifier_DGL under ONE
        backward of loss_f + alpha (loss_a + loss_v).  detach_fused=False (concat and sum heads): loss_f also reaches the encoders.
        Both False: the multi-task baseline of main.py:177, `alpha` being the scripts' --gamma.
        diversity: main.py's feature-diversity monitor ("Audio similar / Visual similar", :77-89, :183-184, :356) -- True: each
        encoder's value is computed right behind its training forward on that encoder's own stream, in every form of the step;
        `read()` gains `a_diversity` / `v_diversity`, `epoch_diversity()` returns the means since its last reset.  Off (the
        default) nothing is allocated or launched.  With a process group the values are the LOCAL rank's (the script's
        DataParallel averages over the gathered batch = the mean of the ranks' values at equal local batches).  The Swin visual
        branch returns pooled tokens, no map: refused there.  Not part of `state_dict()`.
        journal: the scripts' per-step log kept on the device -- the capacity in steps of a ring of rows (gdl.journal.COLUMNS:
        the three losses, total_norm / clip_coef / audio_grad_sum / visual_grad_sum, mean |out_a| / mean |out_v|, the two
        diversity values, OGM's scores / ratio / coefficients), written by one launch behind the update at every step together
        with the epoch's float64 sums; `tr.journal()` is then ONE host copy per epoch where the script synchronises at every
        step (main_dgl.py:132-165).  mode="dgl" feeds the abs_out columns, the joint step has no unimodal logits (NaN; loss_a /
        loss_v are whatever `read()` reports); the diversity columns need diversity=True, the OGM columns a modulated step.
        Every form of the step, the Swin composition and a process group are allowed: with a group the losses and logits are
        the LOCAL rank's and the gradient statistics those of the reduced gradient.  0 (the default): nothing is allocated or
        launched and the step is bit for bit what it was.  Not part of `state_dict()`.
        prototypes: a gdl.Prototypes -- prototypical modal rebalance (PMR, CVPR 2023) on the joint step
        (mode="joint", any of the four heads, ResNet18 encoders, modulation="Normal", no process group).  While
        modulation_starts <= self.epoch <= modulation_ends the step adds beta lossp_a + lam lossp_v to CE(out): lossp_m is the
        cross-entropy of the negated Euclidean distances from encoder m's pooled feature to the class prototypes, and only the
        modality whose summed label probability is behind gets a non-zero coefficient, `alpha`.  gdl_proto_ce runs behind each
        encoder's training forward on that encoder's stream, gdl_proto_apply adds alpha u to that side's feature gradient on the
        main stream between the head's feature gradients and the junction event; the other side's gradient, the head's parameter
        gradients, the logits and `loss_f` (= CE(out)) are those of the plain joint step bit for bit.  `read()` gains `pmr` =
        {score_a, score_v, rho, beta, lam, lossp_a, lossp_v}; the journal's columns are unchanged.  The caller refreshes the
        prototypes once per epoch (`prototypes.update`).  Outside the window, or without prototypes, nothing is allocated or
        launched.  `state_dict()` carries the prototypes' state when they are attached.
        beta: main.py's --beta for a model built with args.pe (the probabilistic-embedding stacks on both ResNet18 encoders; the
        switch is the model having them): gdl.dul.DulStage stands behind each encoder's training forward on that encoder's
        stream and between its feature gradient and its backward, in every form of the step (it is head-independent); the
        loss gains beta (regurize_a + regurize_v), `read()` gains both terms (`loss_f` stays CE(out)), the 8 tensors per
        encoder follow its 60 in the arena and its optimizer group, `seed` and the step count key the noise (or
        `step(..., pe_eps=)` supplies it), valid() uses the pooled eval form.  Refused with the branch: the Swin visual
        branch, a process group, modulation other than "Normal", prototypes.  Without the stacks nothing is allocated or
        launched, and a non-zero beta is refused.
        pareto, pareto_scale: MMPareto gradient integration (ICML 2024) on the multi-task step -- mode="dgl",
        detach_fused=False, drop_head_uni=False, the concat or sum head, ResNet18 encoders, at most 512 classes; everything else
        is refused.  Per encoder the step takes two backwards of its one training forward -- from df_m = g_f W_e (the fused
        loss) into the gradient arena and from df_u = g_e W_e (alpha times its own unimodal loss) into a second, trainer-owned
        arena [audio | visual] -- and gdl_pareto_integrate over the encoder's 60 tensors as one vector, all on that encoder's
        stream: where the two gradients agree (their dot product is positive) the arena receives the min-norm combination
        rescaled to the norm of the plain sum, elsewhere the plain sum, times `pareto_scale`.  The head keeps the plain
        multi-task gradient; the clip and the update follow on the integrated arena.  No value is read back; `read()` gains
        `pareto` = {"audio": {S_mm, S_uu, S_mu, gamma, w_m, w_u, s, branch}, "visual": {...}}.  The logits, the losses and the
        BatchNorm buffers of a step are those of the plain multi-task step bit for bit.  `state_dict()` records the switch and the
        scale; a checkpoint of another switch or scale is refused.  Off
        (the default) nothing is allocated, launched or changed."""
        self._check_optimizer(optimizer)
        self._check_modulation(modulation)
        self._check_journal(journal)
        self.pareto, self.pareto_scale = bool(pareto), float(pareto_scale)
        if self.pareto:
            self._check_pareto(mode, detach_fused, drop_head_uni, process_group, prototypes, modulation, beta, self.pareto_scale)
        self._check_prototypes(prototypes, mode, modulation, process_group)
        from .dul import N_DUL, has_stacks

        self.pe = has_stacks(model.audio_net) or has_stacks(model.visual_net)
        if self.pareto and self.pe:
            raise L.GdlError("DGLTrainer: pareto=True beside the probabilistic-embedding branch (a model built with args.pe) is not "
                             "built")
        self.beta = float(beta)
        if self.pe:  # what the branch is not built for is refused before anything is touched, never ignored
            if not (has_stacks(model.audio_net) and has_stacks(model.visual_net)):
                raise L.GdlError("DGLTrainer: the probabilistic-embedding branch needs its stacks on both encoders (ResNet18 built "
                                 "with args.pe); the Swin visual branch has none")
            if process_group is not None:
                raise L.GdlError("DGLTrainer: the probabilistic-embedding branch with a process group is not built")
            if modulation != "Normal":
                raise L.GdlError(f"DGLTrainer: the probabilistic-embedding branch with modulation={modulation!r} is not built (OGM's "
                                 "rule \"4-D tensors\" would catch the new 1x1 weights); modulation must be \"Normal\"")
            if prototypes is not None:
                raise L.GdlError("DGLTrainer: the probabilistic-embedding branch with prototypes is not built")
            if not 0 <= int(seed) < 2 ** 63:
                raise ValueError("DGLTrainer: seed must be in [0, 2**63)")
        elif self.beta != 0.0:
            raise L.GdlError("DGLTrainer: beta weighs the probabilistic-embedding regulariser, and this model has no such stacks "
                             "(build it with args.pe = 1)")
        ne = self.ne = 60 + (N_DUL if self.pe else 0)  # arena tensors per ResNet18 encoder
        self.model = model
        self.mode = mode
        self.alpha = float(alpha)
        self.pg = process_group
        # visual_side_stream: None = the visual encoder's weight gradients get a stream of their own unless a process group is
        # given (the collective's stream is then the fourth); True / False force it.  Measured with a ONE-rank RCCL group on one
        # MI355X (bench.py, GDL_BENCH_FORCE_PG=1): 6.05 ms without, 5.80 ms with it (5.78 ms without a group) -- but a one-rank
        # all-reduce launches no kernel, so whether five streams hold up beside real RCCL traffic is for the first multi-GPU run
        # to tell (bench.py --side-stream on).
        self.visual_side_stream = visual_side_stream
        # early_backward: None = on where it applies (DGL step with the concat (512 + 512) or sum head): each encoder's feature
        # gradient comes from ITS auxiliary loss alone (main_dgl.py:110-122), so gdl_head_uni_dfeat computes it on the encoder's
        # own stream right behind its forward and the backward starts without waiting for the other encoder; the fusion
        # head (logits of all three sets, the losses, fc_out's gradient) follows on the audio stream behind the audio backward.
        # Same numbers bit for bit (tests/test_step_gpu.py::test_early_backward_identical), no forward -> head -> backward junction.
        # With a process group the early form issues the collectives in the order audio_l4, visual_l4, audio_rest, fusion,
        # visual_rest (over two streams; the same host code, hence the same order, on every rank).  Round 5: it is the default
        # there too -- the one-rank proxy reads 5.85 against 5.92 ms (round 4), with emulated collective traffic on a stream of
        # its own 6.18-6.19 against 6.30-6.31 ms (tools/pg_variants.py --emulate-traffic 16, profiles/r05_pg_variants.txt); the
        # two- and four-rank step tests (tests/test_ddp_gpu.py) run both forms against the oracle.  `bench.py --gpus N` still
        # times every variant on first contact with real RCCL traffic (comm.schedule_variants_ms); early_backward=False opts out.
        self.early_backward = early_backward
        if early_backward is None and os.environ.get("GDL_TUNING") == "1" and os.environ.get("GDL_EARLY_BWD") == "0":
            self.early_backward = False  # tuning aid (A/B)
        self.dtype = dtype if dtype is not None else model.audio_net.gdl_dtype
        head = model.fusion_module
        # head kind: concat (fc_out [n,1024]; ConcatFusion / ConcatFusion_DGL) or sum (fc_x, fc_y [n,512]; SumFusion(_DGL))
        # or gated (fc_x, fc_y [512,512] + fc_out [n,512]; GatedFusion_DGL -- the DGL step never gives fc_x / fc_y a
        # gradient (main_dgl.py:114-122 drops phase 1's, loss_f sees detached hidden vectors), so like fc_auxi they stay
        # outside the optimised arena; GatedFusion in the joint step trains all six)
        # or film (fc [512, 262144] + fc_out [n,512]; FiLM(_DGL): all four tensors are trained by the fused loss)
        self.head = ("gated" if hasattr(head, "fc_out") else "sum") if hasattr(head, "fc_x") else \
            ("film" if hasattr(head, "fc") else "concat")
        first = head.fc_x if self.head == "sum" else head.fc_out
        device = first.weight.device
        if device.type != "cuda":
            raise L.GdlError("DGLTrainer: the model must live on an MI355X (cuda) device; there is no CPU path")
        # mode: "dgl" = the step of main_dgl.py; "joint" (or its older name "concat") = the single-loss step of the jointly
        # trained model (main.py:161-175): every head tensor and both encoders learn from CE(out) alone
        self.joint = mode != "dgl"
        self.detach_fused, self.drop_head_uni = bool(detach_fused), bool(drop_head_uni)
        self.ablation = not (self.detach_fused and self.drop_head_uni)
        # tuning aid (A/B, honoured only with GDL_TUNING=1): GDL_MTL_FUSED=0 = the three-launch junction of the detach_fused=False step
        self.mtl_fused = not (os.environ.get("GDL_TUNING") == "1" and os.environ.get("GDL_MTL_FUSED") == "0")
        # GatedFusion_DGL's fc_x / fc_y receive a gradient from the unimodal losses once those are kept (drop_head_uni=False):
        # all six tensors then live in the arena, fc_out behind them (named_parameters() order, as in the joint gated step)
        gated_all = self.head == "gated" and (self.joint or (mode == "dgl" and not self.drop_head_uni))
        self._go = 4 if gated_all and not self.joint else 0  # where fc_out sits among the DGL gated step's arena tensors
        self.x_gate = bool(getattr(head, "x_gate", True))
        if self.head == "gated" and not self.x_gate and not self.joint:
            raise L.GdlError("DGLTrainer: GatedFusion_DGL is built for x_gate=True (basic_model.py:38)")
        self.n_classes = (head.fc_out if self.head == "gated" else first).weight.shape[0]
        # ---- flat arenas: [trained fusion-head tensors | audio_net (60) | visual_net (60)]
        # (ConcatFusion_DGL's fc_auxi never receives a gradient, SURVEY G1: it stays outside the arena)
        if self.head == "film":
            named = [("fusion_module.fc.weight", head.fc.weight), ("fusion_module.fc.bias", head.fc.bias),
                     ("fusion_module.fc_out.weight", head.fc_out.weight), ("fusion_module.fc_out.bias", head.fc_out.bias)]
        elif self.head == "sum" or gated_all:
            named = [("fusion_module.fc_x.weight", head.fc_x.weight), ("fusion_module.fc_x.bias", head.fc_x.bias),
                     ("fusion_module.fc_y.weight", head.fc_y.weight), ("fusion_module.fc_y.bias", head.fc_y.bias)]
            if self.head == "gated":  # all six tensors are trained (named_parameters() order)
                named += [("fusion_module.fc_out.weight", head.fc_out.weight), ("fusion_module.fc_out.bias", head.fc_out.bias)]
        else:
            named = [("fusion_module.fc_out.weight", head.fc_out.weight), ("fusion_module.fc_out.bias", head.fc_out.bias)]
        nf = self.nf = len(named)
        named += [("audio_net." + n, p) for n, p in model.audio_net.named_parameters()]
        named += [("visual_net." + n, p) for n, p in model.visual_net.named_parameters()]
        # the visual branch: ResNet18 (60 tensors, 512 features) or the Swin composition of SURVEY row N4
        # (models.basic_model.AVClassifier_DGL_Swin: gdl.swin.SwinEngine, num_features wide)
        self.vis_swin = hasattr(model.visual_net, "cfg") and hasattr(model.visual_net, "num_features")
        self.nv = len(named) - nf - ne
        self.dv = int(model.visual_net.num_features) if self.vis_swin else 512
        self.prototypes = prototypes
        self._pmr_now = False
        self._pmr_B = None  # the batch size the step's PMR buffers were allocated for (None: none yet)
        if prototypes is not None:
            if self.vis_swin:
                raise L.GdlError("DGLTrainer: prototypes are not built for the Swin visual branch (768 features; the prototypes "
                                 "are 512 wide)")
            if prototypes.n_classes != self.n_classes:
                raise L.GdlError(f"DGLTrainer: the prototypes hold {prototypes.n_classes} classes, the model's head {self.n_classes}")
            if prototypes.device != device:
                raise L.GdlError(f"DGLTrainer: the prototypes are on {prototypes.device}, the model on {device}")
        if self.pareto:  # (what depends on the model; the switches were checked before it was touched)
            if self.vis_swin:
                raise L.GdlError("DGLTrainer: pareto=True is not built for the Swin visual branch (ResNet18 encoders only)")
            if self.head not in ("concat", "sum"):
                raise L.GdlError(f"DGLTrainer: pareto=True is built for the concat and sum heads, not for {self.head!r} (its fused "
                                 "path into the features needs kernels of its own)")
            if self.n_classes > 512:
                raise L.GdlError(f"DGLTrainer: pareto=True handles at most 512 classes (gdl_head_mtl_ce), the head has {self.n_classes}")
        if self.vis_swin and (self.head != "concat" or mode != "dgl"):
            raise L.GdlError("DGLTrainer: the Swin visual branch is built for the concat DGL head")
        if not self.vis_swin and self.nv != ne:
            raise L.GdlError("DGLTrainer: visual_net must be the ResNet18 mirror or the SwinTransformer mirror")
        if self.ablation:
            if mode != "dgl":  # the joint step has one loss and nothing to truncate: never silently ignored
                raise L.GdlError("DGLTrainer: detach_fused / drop_head_uni switch the truncations of the DGL step (mode=\"dgl\"); "
                                 f"the {mode!r} step has none")
            if self.vis_swin:
                raise L.GdlError("DGLTrainer: the DGL ablation switches are not built for the Swin visual branch")
            if process_group is not None:
                raise L.GdlError("DGLTrainer: the DGL ablation switches with a process group are not supported (the collective "
                                 "order of their steps has not been validated)")
            if not self.detach_fused and self.head not in ("concat", "sum"):
                raise L.GdlError(f"DGLTrainer: detach_fused=False is built for the concat and sum heads, not for {self.head!r} (its "
                                 "fused path into the features needs kernels of its own)")
        if diversity and self.vis_swin:
            raise L.GdlError("DGLTrainer: diversity=True needs each encoder's final feature map [N, 512, h, w]; the Swin visual "
                             "branch has none (its encoder returns pooled tokens)")
        self.modulation = modulation
        self.modulation_starts, self.modulation_ends = int(modulation_starts), int(modulation_ends)
        self.seed = int(seed)
        self.epoch = 0  # the caller sets it per epoch: the modulation's window (main.py:290)
        if modulation != "Normal":
            if not self.joint:  # main_dgl.py parses --modulation and never reads it: not silently ignored here
                raise L.GdlError("DGLTrainer: gradient modulation belongs to the joint step (mode=\"joint\", main.py); "
                                 "main_dgl.py's step has none")
            if self.vis_swin:
                raise L.GdlError("DGLTrainer: gradient modulation is not built for the Swin visual branch")
            if self.head not in ("concat", "sum"):
                raise L.GdlError(f"DGLTrainer: OGM's unimodal logits are defined for the concat and sum heads, not for {self.head!r}")
            if process_group is not None:
                raise L.GdlError("DGLTrainer: gradient modulation with a process group is not supported (the scores would need "
                                 "a collective of their own)")
            if not 0 <= self.seed < 2 ** 63:
                raise ValueError("DGLTrainer: seed must be in [0, 2**63)")
        group = [0] * nf + [1] * ne + [2] * self.nv
        super().__init__(named, group, device, optimizer, lr, momentum, weight_decay, max_norm)
        if modulation != "Normal":  # every 4-D tensor (convolution weight) of the two encoders; BatchNorm and the head untouched
            self._setup_modulation([g if p.dim() == 4 else 0 for g, (_, p) in zip(group, named)], modulation == "OGM_GE",
                                   self.alpha, self.seed)
            self.score_ws = torch.zeros(max(self.lib.gdl_head_uni_scores_workspace_bytes(), 4), dtype=torch.uint8, device=device)
        offs = self.offsets
        # all-reduce buckets (ranges of the flat gradient arena).  layer4 = the last 15 tensors of an encoder, 8.4 M
        # of its 11.2 M parameters, is final right after the first two blocks of the backward: its own bucket lets
        # three quarters of the exchange overlap the rest of the backward.
        a0, v0 = nf, nf + ne
        # (Swin: the last stage + final norm -- the tensors whose gradients the backward finishes first, SwinEngine.backward
        # phase 1 -- play layer4's part)
        vsplit = v0 + 45 if not self.vis_swin else \
            v0 + next(i for i, (n, _) in enumerate(named[v0:]) if n.startswith("visual_net.layers.%d." % (model.visual_net.num_layers - 1)))
        self.bucket = {"fusion": (0, offs[nf]),
                       "audio_l4": (offs[a0 + 45], offs[a0 + ne]), "audio_rest": (offs[a0], offs[a0 + 45]),
                       "visual_l4": (offs[vsplit], offs[v0 + self.nv]), "visual_rest": (offs[v0], offs[vsplit])}
        if process_group is not None:
            from .ddp import BucketReducer

            self.reducer = BucketReducer(self.grads, self.bucket, process_group, backend=comm_backend)
            self.world = self.reducer.world
            # Replica state follows rank 0 (parameters, momentum, BatchNorm running statistics / counters): a seed
            # that differs between ranks or a rank-0-only checkpoint load must not diverge silently.  fc_auxi (and the
            # gated head's fc_x / fc_y) live outside the arena: they are never updated but still part of the state.
            self.reducer.sync_state([self.params] + list(self._opt_state().values()) + self._replica_buffers())
        self.losses = torch.zeros(3, device=self.device)  # loss_f, loss_a, loss_v
        if self.pareto:
            # the second gradient arena [audio | visual] (the unimodal losses' gradients, laid out like the encoders' part of the
            # first), an info row and a workspace per encoder
            e0, e1, e2 = offs[nf], offs[nf + ne], offs[nf + 2 * ne]
            self.pareto_grads = torch.zeros(e2 - e0, device=self.device)
            self.pareto_gviews = [self.pareto_grads[offs[i] - e0:offs[i + 1] - e0].view(named[i][1].shape)
                                  for i in range(nf, nf + 2 * ne)]
            self.pareto_range = ((e0, e1 - e0), (e1, e2 - e1))  # (offset in the gradient arena, elements) per encoder
            self.pareto_info = torch.zeros((2, 8), device=self.device)
            self.pareto_ws = [torch.empty(self.lib.gdl_pareto_workspace_bytes(n_), dtype=torch.uint8, device=self.device)
                              for _, n_ in self.pareto_range]
        if diversity:
            self._setup_diversity(("a_diversity", "v_diversity"))
        self._setup_journal(journal, self.mode == "dgl")
        self.eng_a = self.eng_v = None
        self.dul = None  # (audio stage, visual stage) once the batch shape is known
        self._pe_eps = (None, None)

    @staticmethod
    def _check_prototypes(prototypes, mode, modulation, process_group):
        """(like `_check_optimizer`: before the model is touched) what prototypical modal rebalance is not built for is refused,
        never ignored; the checks against the model -- class count, device, the Swin branch -- follow once the head is known."""
        if prototypes is None:
            return
        from .prototypes import Prototypes

        if not isinstance(prototypes, Prototypes):
            raise L.GdlError(f"DGLTrainer: prototypes must be a gdl.Prototypes, got {type(prototypes).__name__}")
        if mode == "dgl":
            raise L.GdlError("DGLTrainer: prototypes belong to the joint step (mode=\"joint\"); the DGL step has no fused loss in "
                             "its encoders for the prototype term to rebalance")
        if modulation != "Normal":
            raise L.GdlError(f"DGLTrainer: prototypes with modulation={modulation!r} are not built (two rebalancing methods in one "
                             "step); modulation must be \"Normal\"")
        if process_group is not None:
            raise L.GdlError("DGLTrainer: prototypes with a process group are not supported (the scores are sums over the global "
                             "batch and would need a collective of their own)")

    @staticmethod
    def _check_pareto(mode, detach_fused, drop_head_uni, process_group, prototypes, modulation, beta, scale):
        """(like `_check_optimizer`: before the model is touched) MMPareto integration is built for ONE step, the multi-task one;
        every other configuration is refused with its reason, never ignored.  The checks against the model -- the head, the Swin
        branch, the probabilistic-embedding stacks, the class count -- follow once it is known."""
        if mode != "dgl":
            raise L.GdlError(f"DGLTrainer: pareto=True integrates the fused and the unimodal gradients of the multi-task step "
                             f"(mode=\"dgl\", detach_fused=False, drop_head_uni=False); the {mode!r} step has one loss")
        if detach_fused or drop_head_uni:
            raise L.GdlError("DGLTrainer: pareto=True needs both DGL truncations lifted (detach_fused=False, drop_head_uni=False): "
                             f"got detach_fused={bool(detach_fused)}, drop_head_uni={bool(drop_head_uni)} -- with the fused logits "
                             "detached no fused gradient reaches the encoders")
        if process_group is not None:
            raise L.GdlError("DGLTrainer: pareto=True with a process group is not built (the three sums would need a collective of "
                             "their own)")
        if beta != 0.0:
            raise L.GdlError("DGLTrainer: pareto=True with beta (the probabilistic-embedding regulariser) is not built")
        if prototypes is not None:
            raise L.GdlError("DGLTrainer: pareto=True with prototypes is not built (two rebalancing methods in one step)")
        if modulation != "Normal":
            raise L.GdlError(f"DGLTrainer: pareto=True with modulation={modulation!r} is not built (two rebalancing methods in one "
                             "step); modulation must be \"Normal\"")
        if not (scale == scale and abs(scale) != float("inf")):
            raise ValueError(f"DGLTrainer: pareto_scale must be a finite number, got {scale!r}")

    def _journal_logits(self):
        return (self.out_a, self.out_v) if self.mode == "dgl" else (None, None)

    def _replica_buffers(self):
        """Every tensor of the replica that is not in the flat arenas: BatchNorm running statistics and counters of
        both encoders, and the fusion-head parameters the step never trains."""
        m = self.model
        in_arena = {v.data_ptr() for v in getattr(self, "pviews", [])}
        extra = [p.data for p in m.fusion_module.parameters() if p.data.data_ptr() not in in_arena]
        return [b for net in (m.audio_net, m.visual_net) for b in net.buffers()] + extra

    def sync_replicas(self):
        """Broadcast rank 0's BatchNorm buffers (before eval / checkpoint: 'replica 0 persists', main_dgl.py:244 --
        BatchNorm statistics are per rank during training, as with the reference's nn.DataParallel replicas)."""
        if self.reducer is not None:
            self.reducer.broadcast_buffers(self._replica_buffers())

    def state_dict(self):
        """In data-parallel mode the BatchNorm buffers are first made rank 0's, so model.state_dict() taken next is the
        reference's replica-0 state."""
        self.sync_replicas()
        sd = super().state_dict()
        if self.modulation != "Normal":  # (main.py's checkpoints record --modulation and assert on it at load)
            sd.update(modulation=self.modulation, seed=self.seed)
        if self.ablation:  # (the arena's composition and the step depend on them)
            sd.update(detach_fused=self.detach_fused, drop_head_uni=self.drop_head_uni)
        if self.prototypes is not None:  # (the step's loss depends on them; they carry an epoch-to-epoch momentum)
            sd["prototypes"] = self.prototypes.state_dict()
        if self.pareto:  # (the encoders' gradient depends on it)
            sd.update(pareto=True, pareto_scale=self.pareto_scale)
        return sd

    def load_state_dict(self, sd):
        kind = sd.get("modulation", "Normal")
        if kind != self.modulation:
            raise L.GdlError(f"DGLTrainer.load_state_dict: the checkpoint was trained with modulation {kind!r}, this trainer "
                             f"runs {self.modulation!r}")
        sw = (bool(sd.get("detach_fused", True)), bool(sd.get("drop_head_uni", True)))
        if sw != (self.detach_fused, self.drop_head_uni):
            raise L.GdlError(f"DGLTrainer.load_state_dict: the checkpoint was trained with detach_fused={sw[0]}, drop_head_uni={sw[1]}, "
                             f"this trainer runs detach_fused={self.detach_fused}, drop_head_uni={self.drop_head_uni}")
        if bool(sd.get("pareto", False)) != self.pareto:
            raise L.GdlError("DGLTrainer.load_state_dict: the checkpoint was trained " + ("with" if sd.get("pareto", False) else "without") +
                             " pareto integration, this trainer runs " + ("without" if sd.get("pareto", False) else "with") + " it")
        if self.pareto and float(sd.get("pareto_scale", 1.0)) != self.pareto_scale:  # (it scales the encoders' gradient)
            raise L.GdlError(f"DGLTrainer.load_state_dict: the checkpoint was trained with pareto_scale={float(sd.get('pareto_scale', 1.0))!r}, "
                             f"this trainer runs pareto_scale={self.pareto_scale!r}")
        if ("prototypes" in sd) != (self.prototypes is not None):
            raise L.GdlError("DGLTrainer.load_state_dict: the checkpoint was trained " + ("with" if "prototypes" in sd else "without") +
                             " prototypes, this trainer runs " + ("without" if "prototypes" in sd else "with") + " them")
        super().load_state_dict(sd)
        if self.prototypes is not None:
            self.prototypes.load_state_dict(sd["prototypes"])
        if self._mod is not None:  # the noise continues the checkpoint's stream: its key, and the step count loaded above
            self.seed = int(sd.get("seed", self.seed))
            self._mod = self._mod[:2] + (self.seed,)
        if self.reducer is not None:  # the model's parameters alias the arena: whatever rank 0 loaded is the truth
            # (the step count too: the Adam bias corrections are derived from it; and the learning rate)
            hp = torch.tensor([self.lr, float(self.steps)], dtype=torch.float64, device=self.device)
            self.reducer.sync_state([self.params] + list(self._opt_state().values()) + self._replica_buffers() + [hp])
            self.lr, self.steps = float(hp[0].item()), int(hp[1].item())

    # ------------------------------------------------------------------ setup per batch shape
    def _prepare(self, spec, image):
        B, F_, T_ = spec.shape
        Bv, C, T, H, W = image.shape
        if Bv != B or C != 3:
            raise L.GdlError("DGLTrainer.step: spec must be [B,F,T'] and image [B,3,T,H,W]")
        key = (B, F_, T_, T, H, W)
        if getattr(self, "_key", None) == key:
            return
        self._key = key
        self.eng_a = EncoderEngine("audio", self.dtype, B, 1, F_, T_, self.device)
        if self.vis_swin:
            cfg = self.model.visual_net.cfg
            if H != cfg["img"] or W != cfg["img"]:
                raise L.GdlError(f"DGLTrainer.step: the Swin branch was built for {cfg['img']} x {cfg['img']} frames")
            self.eng_v = _SwinAdapter(cfg, self.dtype, B, T, self.device, self.model.visual_net)
        else:
            self.eng_v = EncoderEngine("visual", self.dtype, B, T, H, W, self.device)
        # A fourth stream for the visual (critical-path) encoder's weight gradients -- but never a fifth:
        # with a process group the collective's stream is the fourth (see gdl_encoder_side_stream).
        # (tuning aid, honoured only with GDL_TUNING=1: GDL_SIDE_STREAM 0 = off, 1 = both engines)
        side = os.environ.get("GDL_SIDE_STREAM") if os.environ.get("GDL_TUNING") == "1" else None
        if side == "1":
            self.eng_a.side_stream(True)
        # The audio engine's weight gradients ride on the stream step() is called on: that stream only orders the step before and
        # behind, so its hardware queue idles for the whole step -- a fourth lane without a fifth queue (round 4: 5.63 -> 5.43 ms;
        # the audio chain, a quarter of the arithmetic in ~100 small launches, had been the last to finish: 5.36 ms against the
        # visual chain's 5.18, tools/chain_timeline.py).  Bound per step (the caller's current stream may change): step().
        # Not with a process group by default: there the backward runs in two phases without the early start and the visual
        # engine keeps its weight gradients on its chain, and the one-rank proxy (GDL_BENCH_FORCE_PG=1) reads 5.87 ms with the
        # borrowed lane against 5.78 without (5.61 with the visual side stream alone) -- `bench.py --gpus N` times the variants on
        # first contact with real RCCL traffic (`comm.schedule_variants_ms`); `trainer.audio_on_caller` may be set at any time.
        # (tuning aid: GDL_SIDE_STREAM=2 = the round-3 layout, the visual engine's side stream alone; 3 = the borrowed lane forced)
        self.audio_on_caller = side == "3" or (side not in ("0", "1", "2", "4") and self.reducer is None)
        # The borrowed lane for the VISUAL engine instead (tuning aid "4"; a variant `bench.py --gpus N` times): without a group it
        # equals an owned side stream (5.57 ms), with a one-rank group it reads 6.57 ms -- not a default anywhere.
        self.visual_on_caller = side == "4"
        assert not (self.audio_on_caller and self.visual_on_caller), "the caller's stream carries ONE engine's weight gradients"
        want_v = self.visual_side_stream if self.visual_side_stream is not None else self.reducer is None
        if (side in ("1", "2") or (side in (None, "3") and want_v)) and not self.vis_swin:
            self.eng_v.side_stream(True)
        n, d = self.n_classes, self.device
        self.fa, self.fv = torch.empty((B, 512), device=d), torch.empty((B, self.dv), device=d)
        self.dfa, self.dfv = torch.empty((B, 512), device=d), torch.empty((B, self.dv), device=d)
        self.dscr_a, self.dscr_v = torch.empty((B, 512), device=d), torch.empty((B, self.dv), device=d)
        if self.head == "film":
            if B > 512:
                raise L.GdlError("DGLTrainer: the FiLM head handles at most 512 samples per step")
            self.hidden = torch.empty((B, 512) if self.joint else (3, B, 512), device=d)  # joint: h_f alone
            self.head_ws = torch.empty(self.lib.gdl_head_film_workspace_bytes(B), dtype=torch.uint8, device=d)
        if self.head == "gated":  # hidden vectors (saved for the backward) + its scratch
            self.hx, self.hy = torch.empty((B, 512), device=d), torch.empty((B, 512), device=d)
            self.head_ws = torch.empty(2 * B * 512, device=d)
        self.out, self.out_a, self.out_v = (torch.empty((B, n), device=d) for _ in range(3))
        self.g_f, self.g_a, self.g_v = (torch.empty((B, n), device=d) for _ in range(3))
        if not self.detach_fused:  # gdl_head_mtl_ce's ticket counter and loss terms: zeroed here once, left zero by every launch
            self.mtl_ws = torch.zeros(self.lib.gdl_head_mtl_ce_workspace_bytes(B), dtype=torch.uint8, device=d)
        if self.pareto:  # df_m = g_f W_e, the fused loss' feature gradients (self.dfa / self.dfv hold df_u)
            self.dfm_a, self.dfm_v = torch.empty((B, 512), device=d), torch.empty((B, 512), device=d)
        if self._mod is not None:
            if n > 512:
                raise L.GdlError("DGLTrainer: gradient modulation handles at most 512 classes")
            self.mod_prob = torch.empty((B, 2), device=d)  # softmax(out_a)[label], softmax(out_v)[label] per sample
        self.B = B
        if self.pe:
            from .dul import DulStage

            nf, ne = self.nf, self.ne
            self.dul = (DulStage(self.model.audio_net, self.eng_a, self.pviews[nf + 60:nf + ne], self.gviews[nf + 60:nf + ne]),
                        DulStage(self.model.visual_net, self.eng_v, self.pviews[nf + ne + 60:nf + 2 * ne],
                                 self.gviews[nf + ne + 60:nf + 2 * ne]))
            self.fa_raw, self.fv_raw = torch.empty((B, 512), device=d), torch.empty((B, 512), device=d)  # valid()

    def _bind(self):
        m = self.model
        if self.vis_swin:
            self.eng_v.set_params([p.data for p in m.visual_net.parameters()])
        for eng, net in ((self.eng_a, m.audio_net),) + (() if self.vis_swin else ((self.eng_v, m.visual_net),)):
            bns = net._bn_layers()
            eng.set_params([p.data for p in net.engine_parameters()], [b.running_mean for b in bns],
                           [b.running_var for b in bns], [b.num_batches_tracked for b in bns])

    def _enc_forward(self, m, x):
        """Encoder m's (0 audio, 1 visual) training forward into self.fa / self.fv on the current stream -- with the
        probabilistic-embedding branch: the engine up to its final map, then the stage."""
        eng, f = (self.eng_a, self.fa) if m == 0 else (self.eng_v, self.fv)
        if not self.pe:
            eng.forward(x, True, feat_out=f)
            return
        _, fmap = eng.forward(x, True, want_feat=False, want_fmap=True)
        self.dul[m].forward(fmap, f, self.seed, self.steps, self._pe_eps[m])

    # ------------------------------------------------------------------ the step
    def step(self, spec, image, label, pe_eps=None):
        """spec [B,F,T'] float, image [B,3,T,H,W] float, label [B] int64 -- all resident on the device.
        pe_eps: with the probabilistic-embedding branch, an optional pair (audio, visual) of caller-supplied float32 noise maps
        [n_img P, 512] in the engine's row order ([n_img][P], e.g. torch.randn of the NCHW map permuted to NHWC), used bit for
        bit in place of the generator's; either entry may be None."""
        self._prepare(spec, image)
        self._check_label(label)
        self._bind()
        if pe_eps is not None and not self.pe:
            raise L.GdlError("DGLTrainer.step: pe_eps given, but the model has no probabilistic-embedding stacks")
        self._pe_eps = (None, None) if pe_eps is None else (self.dul[0].check_eps(pe_eps[0]), self.dul[1].check_eps(pe_eps[1]))
        # The head, the losses and the optimizer run on the audio chain's stream rather than on the caller's: one stream
        # (hardware queue) less in play measured +1 % (tools: 9 660 -> 9 760 samples/s).  The caller's stream is ordered
        # before the step and behind it, so the call keeps ordinary stream semantics.
        caller = torch.cuda.current_stream(self.device)
        main = self.s_a
        # the borrowed lane (the stream this call came in on): the audio engine's weight gradients, or the visual engine's
        if self.audio_on_caller:
            self.eng_a.borrow_side_stream(caller.cuda_stream)
        elif isinstance(self.eng_a.lane(), tuple):
            self.eng_a.borrow_side_stream(None)
        if not self.vis_swin:
            if self.visual_on_caller and not self.audio_on_caller:
                self.eng_v.borrow_side_stream(caller.cuda_stream)
            elif isinstance(self.eng_v.lane(), tuple):
                self.eng_v.borrow_side_stream(None)
        main.wait_stream(caller)
        with torch.cuda.stream(main):
            self._step_on(main, spec, image, label)
        caller.wait_stream(main)

    def _step_on(self, main, spec, image, label):
        audio = spec.unsqueeze(1)  # main_dgl.py:100
        label = label.contiguous()
        B, n = self.B, self.n_classes
        self._mark(main, "start")
        ev = main.record_event()
        self.s_a.wait_event(ev)
        self.s_v.wait_event(ev)
        # the visual encoder is the critical path (3x the audio work): enqueue it first so the single
        # host thread's ~100 launches per encoder pass do not delay it
        dgl = self.mode == "dgl"
        early = (dgl and self.detach_fused and self.head in ("concat", "sum") and n <= 512 and self.early_backward is not False
                 and (self.dv == 512 or (self.head == "concat" and self.dv in (768, 1024))))
        red = self.reducer
        if early:
            wa, wv, ldw, ba, bv = self._uni_operands(self.dv)
            with torch.cuda.stream(self.s_v):
                self._enc_forward(1, image)
                self._diversity(self.eng_v, 1)
                L.call("gdl_head_uni_dfeat_w", L.ptr(self.fv), wv, ldw, bv, L.ptr(label), self.alpha, L.ptr(self.dfv), B, n,
                       self.dv, self.s_v.cuda_stream)
                ev_v = self.s_v.record_event()
            with torch.cuda.stream(self.s_a):
                self._enc_forward(0, audio)
                self._diversity(self.eng_a, 0)
                L.call("gdl_head_uni_dfeat", L.ptr(self.fa), wa, ldw, ba, L.ptr(label), self.alpha, L.ptr(self.dfa), B, n,
                       self.s_a.cuda_stream)
            # (host order: both forwards are enqueued before either backward, so neither chain waits for the host)
            self._encoders_backward()
            # the fusion head on the audio stream (= main), behind the audio backward: all three logit sets, the losses, the
            # gradient of fc_out (/ fc_x, fc_y) from loss_f alone; its feature gradients go to scratch (the encoders have theirs)
            main.wait_event(ev_v)
            st = main.cuda_stream
            self._head_forward(True, st)
            L.call("gdl_softmax_ce3", L.ptr(self.out), L.ptr(self.out_a), L.ptr(self.out_v), L.ptr(label), 1.0, self.alpha,
                   self.alpha, self.losses.data_ptr(), L.ptr(self.g_f), L.ptr(self.g_a), L.ptr(self.g_v), B, n, st)
            self._dgl_head_backward(self.dscr_a, self.dscr_v, st)
            if red is not None:
                red.launch("fusion")
                with torch.cuda.stream(self.s_v):
                    red.launch("visual_rest")
            self._finish_step(main, st)
            return
        pmr = self._pmr_now = (self.prototypes is not None and self.modulation_starts <= self.epoch <= self.modulation_ends)
        if pmr:
            self._pmr_buffers()
        with torch.cuda.stream(self.s_v):
            self._enc_forward(1, image)
            self._diversity(self.eng_v, 1)
            if pmr:
                self._proto_ce(1, self.fv, label, self.s_v.cuda_stream)
        with torch.cuda.stream(self.s_a):
            self._enc_forward(0, audio)
            self._diversity(self.eng_a, 0)
            if pmr:
                self._proto_ce(0, self.fa, label, self.s_a.cuda_stream)
        main.wait_stream(self.s_a)
        main.wait_stream(self.s_v)
        self._mark(main, "fwd_done")
        st = main.cuda_stream
        if dgl and not self.detach_fused:
            if self.pareto:
                # the unimodal losses' feature gradients alone (fused_reaches = 0: self.dfa / self.dfv = df_u), then the fused
                # loss' through the head, df_m = g_f W_e, into buffers of their own
                self._mtl_junction(label, st, fused_reaches=0)
                self._fused_dfeat(st)
            else:
                self._mtl_junction(label, st)
            self._mark(main, "head_done")
            ev2 = main.record_event()
            self.s_v.wait_event(ev2)
            # the head's parameter gradients behind the junction event, on this stream (= the audio chain, the shorter one) in
            # front of the audio backward, as in the joint step
            self._dgl_head_backward(None, None, st)
            if self.pareto:
                self._pareto_backward()
            else:
                self._encoders_backward()
            self._finish_step(main, st)
            return
        self._head_forward(dgl, st)
        lp = self.losses.data_ptr()
        if dgl:  # loss_f, alpha*loss_a, alpha*loss_v (main_dgl.py:102-108) in one launch
            L.call("gdl_softmax_ce3", L.ptr(self.out), L.ptr(self.out_a), L.ptr(self.out_v), L.ptr(label), 1.0, self.alpha,
                   self.alpha, lp, L.ptr(self.g_f), L.ptr(self.g_a), L.ptr(self.g_v), B, n, st)
        else:
            L.call("gdl_softmax_ce", L.ptr(self.out), L.ptr(label), 1.0, lp, L.ptr(self.g_f), B, n, st)
        if dgl:
            self._dgl_head_backward(self.dfa, self.dfv, st)
        else:  # BASELINE config 1: one CE loss (main.py:161-175) through the head into both encoders
            # Only the feature gradients stand between the head and the encoder backwards.  Without a process group the head's
            # parameter gradients follow behind the junction event, on this stream (= the audio chain, the shorter one) in front
            # of the audio backward; the visual chain, the critical path, starts as soon as dfa / dfv exist.  Same kernels, same
            # numbers.  With a process group the fusion bucket's collective is launched at the junction: everything first.
            self._joint_head_backward(st, True, red is not None)
            if pmr:
                # prototypical modal rebalance: dfa += beta u_a, dfv += lam u_v (one of the two, chosen on the device from the
                # scores), behind the head's feature gradients and in front of the junction event -- the one launch PMR adds to
                # the critical path; the two gdl_proto_ce ran behind the forwards on the encoders' own streams
                L.call("gdl_proto_apply", L.ptr(self.pmr_terms[0]), L.ptr(self.pmr_terms[1]), L.ptr(self.pmr_u[0]),
                       L.ptr(self.pmr_u[1]), L.ptr(self.dfa), L.ptr(self.dfv), self.alpha, L.ptr(self.pmr_stats), B, 512, st)
        self._mark(main, "head_done")
        if red is not None:
            red.launch("fusion")
        ev2 = main.record_event()
        self.s_a.wait_event(ev2)
        self.s_v.wait_event(ev2)
        self._mod_now = (self._mod is not None and self.modulation_starts <= self.epoch <= self.modulation_ends)
        if self._mod_now:
            # OGM's unimodal scores from the pooled features and the head's current parameters (main.py:286-295), behind the
            # head forward on its stream (= the audio chain, the shorter one): the visual backward is not kept waiting
            # concat: out_a = a W[:, :512]^T + b / 2, out_v = v W[:, 512:]^T + b / 2; sum: out_a = fc_x(a), out_v = fc_y(v)
            wa, wv, ldw, ba, bv = self._uni_operands(512)
            bs = 0.5 if self.head == "concat" else 1.0
            L.call("gdl_head_uni_scores", L.ptr(self.fa), L.ptr(self.fv), wa, wv, ldw, ba, bv, bs, L.ptr(label),
                   L.ptr(self.mod_prob), L.ptr(self.mod_scores), B, n, L.ptr(self.score_ws), self.score_ws.numel(), st)
        if not dgl and red is None:
            self._joint_head_backward(st, False, True)
        self._encoders_backward()
        if red is not None:
            with torch.cuda.stream(self.s_v):
                red.launch("visual_rest")
        self._finish_step(main, st)

    def _pmr_buffers(self):
        """What a step with the prototype term writes besides the step's own tensors, allocated at the first such step (and
        again for another batch size): u [2, B, 512], the samples' terms [2, 2, B], stats [8]."""
        if self._pmr_B != self.B:
            d = self.device
            self.pmr_u = torch.empty((2, self.B, 512), device=d)
            self.pmr_terms = torch.empty((2, 2, self.B), device=d)
            self.pmr_stats = torch.zeros(8, device=d)
            self._pmr_B = self.B

    def _proto_ce(self, m, feat, label, st):
        """gdl_proto_ce for modality m (0 audio, 1 visual) behind its encoder's training forward, on that encoder's stream"""
        L.call("gdl_proto_ce", L.ptr(feat), L.ptr(self.prototypes.protos[m]), L.ptr(label), L.ptr(self.pmr_u[m]),
               L.ptr(self.pmr_terms[m]), None, self.B, self.n_classes, 512, st)

    def _uni_operands(self, dv):
        """(wa, wv, ldw, ba, bv): the two modalities' linear maps inside a concat or sum head, for a visual width of dv."""
        pv = self.pviews
        if self.head == "concat":  # fc_out [n][512 + dv] + one bias: the audio columns first
            return L.ptr(pv[0]), pv[0].data_ptr() + 512 * 4, 512 + dv, L.ptr(pv[1]), L.ptr(pv[1])
        return L.ptr(pv[0]), L.ptr(pv[2]), 512, L.ptr(pv[1]), L.ptr(pv[3])  # fc_x, fc_y [n][512] with their biases

    def _encoders_backward(self):
        """Both encoders' backward from self.dfa / self.dfv, the visual one (the critical path) enqueued first.  Data parallel:
        each in two phases so that the layer4 bucket (75 % of the bytes) is exchanged while layer3 .. stem are still being
        differentiated.  Collectives of one communicator run in issue order, identical on every rank: audio before visual (the
        audio passes are the shorter ones) -- audio_l4, visual_l4, audio_rest here; `visual_rest` is the caller's to launch (the
        early form puts `fusion` in front of it)."""
        red, nf = self.reducer, self.nf
        ne = self.ne
        gv, ga = self.gviews[nf + ne:nf + ne + self.nv], self.gviews[nf:nf + ne]
        if self.pe:  # the stage between each feature gradient and its engine's backward, on the same chain
            step = self.steps
            with torch.cuda.stream(self.s_v):
                self.eng_v.backward(gv[:60], dfmap=self.dul[1].backward(self.dfv, self.beta, self.seed, step, self._pe_eps[1]))
            with torch.cuda.stream(self.s_a):
                self.eng_a.backward(ga[:60], dfmap=self.dul[0].backward(self.dfa, self.beta, self.seed, step, self._pe_eps[0]))
            return
        if red is None:
            with torch.cuda.stream(self.s_v):
                self.eng_v.backward(gv, dfeat=self.dfv)
            with torch.cuda.stream(self.s_a):
                self.eng_a.backward(ga, dfeat=self.dfa)
            return
        with torch.cuda.stream(self.s_v):
            self.eng_v.backward(gv, dfeat=self.dfv, phase=1)
        with torch.cuda.stream(self.s_a):
            self.eng_a.backward(ga, dfeat=self.dfa, phase=1)
            red.launch("audio_l4")
        with torch.cuda.stream(self.s_v):
            red.launch("visual_l4")
            self.eng_v.backward(gv, phase=2)
        with torch.cuda.stream(self.s_a):
            self.eng_a.backward(ga, phase=2)
            red.launch("audio_rest")

    def _fused_dfeat(self, st):
        """(pareto) df_m = g_f W_e for both encoders into self.dfm_a / self.dfm_v: the head's backward from g_f alone, feature
        gradients only -- the call the joint step makes for its dfa / dfv."""
        pv, B, n = self.pviews, self.B, self.n_classes
        if self.head == "sum":
            L.call("gdl_head_sum_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[2]), None, None, L.ptr(self.g_f),
                   1, 0, L.ptr(self.dfm_a), L.ptr(self.dfm_v), None, None, None, None, B, n, st)
        else:
            L.call("gdl_head_concat_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), None, None, L.ptr(self.g_f), 1, 0,
                   L.ptr(self.dfm_a), L.ptr(self.dfm_v), None, None, B, n, st)

    def _pareto_backward(self):
        """(pareto) On each encoder's own stream, the visual one (the critical path) enqueued first: the backward of its training
        forward from df_m into the gradient arena's views, the same backward from df_u into the second arena, and
        gdl_pareto_integrate over the encoder's range -- the arena then holds the integrated gradient.  Nothing is read back."""
        nf, ne = self.nf, self.ne
        gm = (self.gviews[nf:nf + ne], self.gviews[nf + ne:nf + 2 * ne])
        gu = (self.pareto_gviews[:ne], self.pareto_gviews[ne:])
        lanes = ((1, self.s_v, self.eng_v, self.dfm_v, self.dfv), (0, self.s_a, self.eng_a, self.dfm_a, self.dfa))
        for m, s, eng, dfm, _ in lanes:  # (host order: both first backwards are enqueued before either second one)
            with torch.cuda.stream(s):
                eng.backward(gm[m], dfeat=dfm)
        e0 = self.pareto_range[0][0]
        for m, s, eng, _, dfu in lanes:
            off, cnt = self.pareto_range[m]
            with torch.cuda.stream(s):
                eng.backward(gu[m], dfeat=dfu)
                L.call("gdl_pareto_integrate", self.grads.data_ptr() + 4 * off, self.pareto_grads.data_ptr() + 4 * (off - e0), cnt,
                       self.pareto_scale, L.ptr(self.pareto_info[m]), L.ptr(self.pareto_ws[m]), self.pareto_ws[m].numel(),
                       s.cuda_stream)

    def _mtl_junction(self, label, st, fused_reaches=1):
        """What stands between the forwards and the backward chains when the fused loss reaches the encoders (concat / sum head):
        the three logit sets, the three losses, their logit gradients and dfa / dfv -- gdl_head_mtl_ce, ONE launch; beyond its 512
        classes (or with the tuning aid GDL_MTL_FUSED=0) the three launches it replaces, bit for bit.  fused_reaches=0 (the
        pareto step, at most 512 classes, always the one launch): dfa / dfv carry the unimodal losses' part alone."""
        B, n = self.B, self.n_classes
        if (self.mtl_fused or not fused_reaches) and n <= 512:
            wa, wv, ldw, ba, bv = self._uni_operands(512)
            sb = 0 if self.head == "concat" else 1  # `out` carries one bias / bx + by
            L.call("gdl_head_mtl_ce", L.ptr(self.fa), L.ptr(self.fv), wa, wv, ldw, ba, bv, sb, L.ptr(label), self.alpha,
                   int(fused_reaches),
                   L.ptr(self.out), L.ptr(self.out_a), L.ptr(self.out_v), self.losses.data_ptr(), L.ptr(self.g_f), L.ptr(self.g_a),
                   L.ptr(self.g_v), L.ptr(self.dfa), L.ptr(self.dfv), B, n, L.ptr(self.mtl_ws), self.mtl_ws.numel(), st)
            return
        self._head_forward(True, st)
        L.call("gdl_softmax_ce3", L.ptr(self.out), L.ptr(self.out_a), L.ptr(self.out_v), L.ptr(label), 1.0, self.alpha,
               self.alpha, self.losses.data_ptr(), L.ptr(self.g_f), L.ptr(self.g_a), L.ptr(self.g_v), B, n, st)
        self._dgl_head_backward(self.dfa, self.dfv, st, par=False)

    def _dgl_head_backward(self, dfa, dfv, st, par=True):
        """The DGL step's head backward; the feature gradients go to `dfa` / `dfv` (None: not computed), `par`: the parameter
        gradients.  DGL truncation: `out` is computed from detached features (out_reaches_xy = 0) and the head gradients of the
        unimodal losses are dropped before loss_f.backward() (uni_in_dw = 0) (main_dgl.py:110-122); `detach_fused` /
        `drop_head_uni` = False lift one or the other."""
        pv, B, n = self.pviews, self.B, self.n_classes
        reach, uni = int(not self.detach_fused), int(not self.drop_head_uni)
        gv = [L.ptr(g) if par else None for g in self.gviews[:self.nf]]
        dfa, dfv = (L.ptr(dfa), L.ptr(dfv)) if dfa is not None else (None, None)
        if self.head == "film":
            L.call("gdl_head_film_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[2]), L.ptr(self.hidden),
                   L.ptr(self.g_a), L.ptr(self.g_v), L.ptr(self.g_f), uni, dfa, dfv, gv[0],
                   gv[1], gv[2], gv[3], B, n, L.ptr(self.head_ws), self.head_ws.numel(), st)
        elif self.head == "gated":
            fm, go = self.model.fusion_module, self._go
            d1 = gv[:4] if go else [None] * 4  # fc_x / fc_y: trained by the unimodal losses alone, when those are kept
            L.call("gdl_head_gated_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(self.hx), L.ptr(self.hy),
                   L.ptr(fm.fc_x.weight), L.ptr(fm.fc_y.weight), L.ptr(pv[go]), L.ptr(self.g_a), L.ptr(self.g_v),
                   L.ptr(self.g_f), uni, dfa, dfv, d1[0], d1[1], d1[2], d1[3], gv[go], gv[go + 1],
                   L.ptr(self.head_ws), B, n, st)
        elif self.head == "sum":
            L.call("gdl_head_sum_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[2]), L.ptr(self.g_a),
                   L.ptr(self.g_v), L.ptr(self.g_f), reach, uni, dfa, dfv, gv[0], gv[1],
                   gv[2], gv[3], B, n, st)
        elif self.dv != 512:  # 512 + num_features wide fc_out (the Swin composition)
            L.call("gdl_head_concat_xy_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(self.g_a), L.ptr(self.g_v),
                   L.ptr(self.g_f), reach, uni, dfa, dfv, gv[0], gv[1], B, n, 512, self.dv, st)
        else:
            L.call("gdl_head_concat_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(self.g_a), L.ptr(self.g_v),
                   L.ptr(self.g_f), reach, uni, dfa, dfv, gv[0], gv[1], B, n, st)

    def _joint_head_backward(self, st, feat, par):
        """The joint step's head backward from self.g_f: `feat` -- dfa / dfv; `par` -- the gradients of every head tensor."""
        pv, B, n = self.pviews, self.B, self.n_classes
        dfa, dfv = (L.ptr(self.dfa), L.ptr(self.dfv)) if feat else (None, None)
        gv = [L.ptr(g) if par else None for g in self.gviews[:self.nf]]
        if self.head == "film":  # fusion_modules.py:91-124
            L.call("gdl_head_film_joint_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[2]), L.ptr(self.hidden),
                   L.ptr(self.g_f), dfa, dfv, gv[0], gv[1], gv[2], gv[3], B, n, L.ptr(self.head_ws), self.head_ws.numel(), st)
        elif self.head == "gated":  # fusion_modules.py:181-210
            L.call("gdl_head_gated_joint_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(self.hx), L.ptr(self.hy), L.ptr(pv[0]),
                   L.ptr(pv[2]), L.ptr(pv[4]), L.ptr(self.g_f), int(self.x_gate), dfa, dfv, gv[0], gv[1], gv[2], gv[3], gv[4],
                   gv[5], L.ptr(self.head_ws), B, n, st)
        elif self.head == "sum":  # fusion_modules.py:5-13
            L.call("gdl_head_sum_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[2]), None, None, L.ptr(self.g_f),
                   1, 0, dfa, dfv, gv[0], gv[1], gv[2], gv[3], B, n, st)
        else:  # fusion_modules.py:33-42
            L.call("gdl_head_concat_bwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), None, None, L.ptr(self.g_f), 1, 0,
                   dfa, dfv, gv[0], gv[1], B, n, st)

    def _head_forward(self, dgl, st):
        """(out, out_a, out_v) from the pooled features self.fa / self.fv."""
        pv, B, n = self.pviews, self.B, self.n_classes
        oa, ov = (L.ptr(self.out_a), L.ptr(self.out_v)) if dgl else (None, None)
        if self.head == "film" and self.joint:  # fusion_modules.py:105-124: the fused form alone
            L.call("gdl_head_film_joint_fwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[1]), L.ptr(pv[2]),
                   L.ptr(pv[3]), L.ptr(self.hidden), L.ptr(self.out), B, n, L.ptr(self.head_ws), self.head_ws.numel(), st)
        elif self.head == "gated" and self.joint:  # fusion_modules.py:198-210 (all six tensors live in the arena)
            L.call("gdl_head_gated_joint_fwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[1]), L.ptr(pv[2]),
                   L.ptr(pv[3]), L.ptr(pv[4]), L.ptr(pv[5]), L.ptr(self.hx), L.ptr(self.hy), L.ptr(self.out), int(self.x_gate),
                   B, n, st)
        elif self.head == "film":  # fusion_modules.py:140-178
            L.call("gdl_head_film_fwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[1]), L.ptr(pv[2]), L.ptr(pv[3]),
                   L.ptr(self.hidden), L.ptr(self.out), oa, ov, B, n, L.ptr(self.head_ws), self.head_ws.numel(), st)
        elif self.head == "gated":  # fusion_modules.py:232-250
            fm = self.model.fusion_module
            L.call("gdl_head_gated_fwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(fm.fc_x.weight), L.ptr(fm.fc_x.bias),
                   L.ptr(fm.fc_y.weight), L.ptr(fm.fc_y.bias), L.ptr(pv[self._go]), L.ptr(pv[self._go + 1]), L.ptr(self.hx),
                   L.ptr(self.hy), L.ptr(self.out), oa, ov, B, n, st)
        elif self.head == "sum":  # fusion_modules.py:22-30
            L.call("gdl_head_sum_fwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[1]), L.ptr(pv[2]), L.ptr(pv[3]),
                   L.ptr(self.out), oa, ov, B, n, st)
        elif self.dv != 512:
            L.call("gdl_head_concat_xy_fwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[1]), L.ptr(self.out), oa, ov,
                   B, n, 512, self.dv, st)
        else:  # fusion_modules.py:38-42 / 51-59
            L.call("gdl_head_concat_fwd", L.ptr(self.fa), L.ptr(self.fv), L.ptr(pv[0]), L.ptr(pv[1]), L.ptr(self.out), oa, ov,
                   B, n, st)

    # ------------------------------------------------------------------ validation (main_dgl.py:168-222)
    def valid(self, batches, bank=None):
        """The reference's valid(): eval-mode forward (BatchNorm running statistics) of every (spec, image, label)
        batch, arg-max of the three logit sets and per-class counters -- all on the device, one host copy at the
        end instead of 3*B per batch.  Returns (acc, acc_a, acc_v) = sum(acc*)/sum(num) as main_dgl.py:222.
        bank: a gdl.ScoreBank (sets = 3 in the DGL mode, 1 for mode="joint") that every batch is appended to behind its
        counters, for mAP / top-k / confusion from `bank.report()`; the return value and `valid_counts` do not change.  A bank
        of another class count, set count or device, or without room for every batch, is refused before the first launch."""
        n = self.n_classes
        if bank is not None:
            batches = list(batches)
            bank.check(n, 3 if self.mode == "dgl" else 1, self.device, sum(int(b[2].shape[0]) for b in batches), "DGLTrainer.valid")
        cnt = torch.zeros((4, n), dtype=torch.int64, device=self.device)
        main = torch.cuda.current_stream(self.device)
        self.sync_replicas()  # data-parallel: evaluate with rank 0's running statistics (SURVEY 8(e) "Buffers")
        for spec, image, label in batches:
            self._prepare(spec, image)
            self._check_label(label)
            self._bind()
            audio = spec.unsqueeze(1)
            label = label.contiguous()
            ev = main.record_event()
            self.s_a.wait_event(ev)
            self.s_v.wait_event(ev)
            with torch.cuda.stream(self.s_v):
                self.eng_v.forward(image, False, feat_out=self.fv_raw if self.pe else self.fv)
                if self.pe:
                    self.dul[1].eval(self.fv_raw, self.fv)
            with torch.cuda.stream(self.s_a):
                self.eng_a.forward(audio, False, feat_out=self.fa_raw if self.pe else self.fa)
                if self.pe:
                    self.dul[0].eval(self.fa_raw, self.fa)
            main.wait_stream(self.s_a)
            main.wait_stream(self.s_v)
            st = main.cuda_stream
            dgl = self.mode == "dgl"
            self._head_forward(dgl, st)
            L.call("gdl_eval_count", L.ptr(self.out), L.ptr(self.out_a) if dgl else None, L.ptr(self.out_v) if dgl else None,
                   L.ptr(label), self.B, n, cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr() if dgl else None,
                   cnt[3].data_ptr() if dgl else None, st)
            if bank is not None:
                bank.append(self.out, self.out_a if dgl else None, self.out_v if dgl else None, label, stream=st)
        c = cnt.cpu().numpy().astype("float64")
        self.valid_counts = c
        tot = max(c[0].sum(), 1.0)
        return c[1].sum() / tot, c[2].sum() / tot, c[3].sum() / tot

    # ------------------------------------------------------------------ results (host sync)
    def read(self):
        """Synchronises and returns the quantities the reference prints / logs per step."""
        r = self._read_stats((self.eng_a, self.eng_v))
        ls = self.losses.cpu().numpy()
        r.update(loss_f=float(ls[0]), loss_a=float(ls[1]), loss_v=float(ls[2]), out=self.out.cpu().numpy())
        if self.mode == "dgl":
            r["out_a"] = self.out_a.cpu().numpy()
            r["out_v"] = self.out_v.cpu().numpy()
        if self.pe:  # main.py's regurize_a / regurize_v of the last step (loss_f above is CE(out) alone)
            r["regurize_a"], r["regurize_v"] = (float(d.reg.cpu().numpy()[0]) for d in self.dul)
        if self._mod is not None and self._mod_now:  # the last step was modulated (the statistics above are the unmodulated ones)
            m = self.mod_stats[:5].cpu().numpy()
            r["ogm"] = dict(score_a=float(m[0]), score_v=float(m[1]), ratio_v=float(m[2]), coeff_a=float(m[3]), coeff_v=float(m[4]))
        if self._pmr_now:  # the last step carried the prototype term (loss_f above is CE(out) alone)
            m = self.pmr_stats.cpu().numpy()
            r["pmr"] = dict(zip(("score_a", "score_v", "rho", "beta", "lam", "lossp_a", "lossp_v"), (float(v) for v in m[:7])))
        if self.pareto:  # the last step's integration per encoder: the three sums (as float), the coefficients, the branch
            keys = ("S_mm", "S_uu", "S_mu", "gamma", "w_m", "w_u", "s", "branch")
            info = self.pareto_info.cpu().numpy()
            r["pareto"] = {k: {**{q: float(v) for q, v in zip(keys[:7], row[:7])}, "branch": int(row[7])}
                           for k, row in zip(("audio", "visual"), info)}
        return self._read_diversity(r)
