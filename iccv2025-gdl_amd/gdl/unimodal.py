"""Native training step of the unimodal baselines: the audio encoder alone or the visual encoder alone with a
`Linear(512, n_classes)` classifier (the reference's models/basic_model.py:46-59, 88-122, `args.modality` 'audio' / 'visual'),
trained by the body of its main.py -- one CrossEntropyLoss on `out`, backward, clip_grad_norm_(.., 40), the optimizer.

Per step (all asynchronous, nothing is read back unless `read()` is called), on the process-wide chain streams of
gdl.trainer (the modality's own as the chain, the other one -- idle here -- as the side lane):
  chain: encoder forward -> gdl_head_cls_ce (logits, loss, dlogits, feature gradient: one launch) -> encoder backward
         -> fused grad statistics -> fused clip + update
  lane : the classifier's dW / db from the stored dlogits (gdl_head_cls_bwd, df = NULL) behind the start of the encoder
         backward, then that backward's weight gradients (gdl_encoder_borrow_side_stream)
The flat arena is [classifier.weight, classifier.bias | the encoder's 60 tensors] with the optimizer groups 0 and 1 (audio)
or 2 (visual), so `audio_grad_sum` / `visual_grad_sum` are the existing statistics and the absent one reads 0.0.  The
`fusion_module` the reference still constructs in these modes gets no gradient: it stays outside the arena, untouched.
A model built with args.pe carries the probabilistic-embedding stacks (main.py --pe 1 --beta b): gdl.dul.DulStage then stands
between the encoder's final map and `f` in the forward, between the head's `df` and the encoder backward in the backward, its 8
tensors follow the encoder's 60 in the arena (same optimizer group), and `read()` gains `regurize_a` / `regurize_v`.
"""
import torch

from . import _lib as L
from .dul import N_DUL, DulStage, has_stacks
from .encoder import EncoderEngine
from .trainer import ArenaTrainer


class UnimodalTrainer(ArenaTrainer):
    """The arenas, the optimizer state and its checkpoint, the statistics + clip + update tail of the step, `grad(name)` and
    `close()` are ArenaTrainer's; here: the 62-tensor list, the step in front of that tail, valid() and read()."""

    _script = "main.py"

    def __init__(self, model, lr, momentum=0.9, weight_decay=None, max_norm=40.0, dtype=None, optimizer="sgd",
                 process_group=None, diversity=False, journal=0, beta=0.0, seed=0):
        """diversity: main.py's feature-diversity monitor (:77-89, :183-184, :356) of this model's one encoder -- True: computed
        right behind the training forward on the chain; `read()` gains `a_diversity` (audio) or `v_diversity` (visual),
        `epoch_diversity()` returns its mean since the last reset.  Off (the default) nothing is allocated or launched.
        journal: the script's per-step log kept on the device, as DGLTrainer's -- the capacity in steps of the ring `tr.journal()`
        hands back with the epoch's means in one host copy.  The script's unimodal model returns `out, out, out`: the one loss
        fills loss_f / loss_a / loss_v and mean |out| both abs_out columns; the absent modality's grad_sum reads 0.0, its
        diversity column NaN.  0 (the default): nothing is allocated or launched.
        beta, seed: main.py's --beta and the key of the branch's noise, for a model built with args.pe (the switch is the model
        having the stacks): the step's loss gains beta * regurize, the noise is a function of (seed, step count, modality,
        element) alone -- or the map `step(..., pe_eps=)` supplies.  beta = 0 is allowed (regurize is still reported).  Without
        the stacks nothing is allocated or launched, and a non-zero beta is refused."""
        self._check_optimizer(optimizer)
        self._check_journal(journal)
        if process_group is not None:
            raise L.GdlError("UnimodalTrainer: data-parallel runs (process_group) are not built for the unimodal baselines")
        modality = getattr(model, "modality", None)
        if modality == "full":
            raise L.GdlError("UnimodalTrainer: modality='full' has both encoders -- use gdl.DGLTrainer (mode='dgl' or 'joint')")
        if modality not in ("audio", "visual"):
            raise L.GdlError(f"UnimodalTrainer: model.modality must be 'audio' or 'visual', got {modality!r}")
        self.modality = modality
        self.mode = "unimodal"
        net = getattr(model, modality + "_net")
        self.pe = has_stacks(net)
        self.beta, self.seed = float(beta), int(seed)
        if not self.pe and self.beta != 0.0:
            raise L.GdlError("UnimodalTrainer: beta weighs the probabilistic-embedding regulariser, and this model has no such "
                             "stacks (build it with args.pe = 1)")
        if self.pe and not 0 <= self.seed < 2 ** 63:
            raise ValueError("UnimodalTrainer: seed must be in [0, 2**63)")
        cls = getattr(model, modality + "_classifier")
        device = cls.weight.device
        if device.type != "cuda":
            raise L.GdlError("UnimodalTrainer: the model must live on an MI355X (cuda) device; there is no CPU path")
        if hasattr(net, "cfg") and hasattr(net, "num_features"):
            raise L.GdlError("UnimodalTrainer: the Swin branch as the only modality is not built (ResNet18 encoders only)")
        if tuple(cls.weight.shape[1:]) != (512,) or cls.weight.shape[0] > 512:
            raise L.GdlError("UnimodalTrainer: the classifier must be Linear(512, n_classes <= 512)")
        self.model, self.net = model, net
        self.dtype = dtype if dtype is not None else net.gdl_dtype
        self.n_classes = cls.weight.shape[0]
        named = [(modality + "_classifier.weight", cls.weight), (modality + "_classifier.bias", cls.bias)]
        named += [(modality + "_net." + n, p) for n, p in net.named_parameters()]
        ne = 60 + (N_DUL if self.pe else 0)
        if len(named) != 2 + ne:
            raise L.GdlError("UnimodalTrainer: the encoder must be the ResNet18 mirror (60 tensors)")
        self.nf = 2
        group = [0, 0] + [1 if modality == "audio" else 2] * ne
        super().__init__(named, group, device, optimizer, lr, momentum, weight_decay, max_norm)
        self.losses = torch.zeros(1, device=self.device)
        self.chain, self.lane = (self.s_a, self.s_v) if modality == "audio" else (self.s_v, self.s_a)
        self.eng = self.dul = None
        if diversity:
            self._setup_diversity(("a_diversity" if modality == "audio" else "v_diversity",))
        self._setup_journal(journal, True)

    def _journal_logits(self):
        return self.out, self.out

    # ------------------------------------------------------------------ setup per batch shape
    def _input(self, spec, image):
        """The encoder's input of a (spec, image) pair; the other modality's tensor is ignored and may be None."""
        x = spec if self.modality == "audio" else image
        want = "spec [B,F,T']" if self.modality == "audio" else "image [B,3,T,H,W]"
        if x is None or x.dim() != (3 if self.modality == "audio" else 5) or (self.modality == "visual" and x.shape[1] != 3):
            raise L.GdlError(f"UnimodalTrainer: the {self.modality} model takes {want}")
        if x.device != self.device:
            raise L.GdlError(f"UnimodalTrainer: the input must be on {self.device}, got {x.device}")
        return x.unsqueeze(1) if self.modality == "audio" else x  # main.py: spec.unsqueeze(1)

    def _prepare(self, x):
        key = tuple(x.shape)
        if getattr(self, "_key", None) == key:
            return
        self._key = key
        B = x.shape[0]
        T, H, W = (1, x.shape[2], x.shape[3]) if self.modality == "audio" else tuple(x.shape[2:])
        self.eng = EncoderEngine(self.modality, self.dtype, B, T, H, W, self.device)
        n, d = self.n_classes, self.device
        self.f, self.df = torch.empty((B, 512), device=d), torch.empty((B, 512), device=d)
        self.out, self.dlogits = torch.empty((B, n), device=d), torch.empty((B, n), device=d)
        self.B = B
        if self.pe:
            self.dul = DulStage(self.net, self.eng, self.pviews[62:], self.gviews[62:])
            self.f_raw = torch.empty((B, 512), device=d)  # valid(): the engine's pooled feature in front of gdl_dul_eval

    def _bind(self):
        bns = self.net._bn_layers()
        self.eng.set_params([p.data for p in self.net.engine_parameters()], [b.running_mean for b in bns],
                            [b.running_var for b in bns], [b.num_batches_tracked for b in bns])

    # ------------------------------------------------------------------ the step
    def step(self, spec, image, label, pe_eps=None):
        """DGLTrainer.step's argument order: spec [B,F,T'] float, image [B,3,T,H,W] float, label [B] int64, resident on the
        device; the tensor of the modality the model does not have may be None.  pe_eps: DGLTrainer.step's pair (audio map,
        visual map) of caller-supplied noise for the probabilistic-embedding branch; the absent modality's entry is ignored."""
        x = self._input(spec, image)
        self._prepare(x)
        self._check_label(label)
        eps = None
        if pe_eps is not None:
            if not self.pe:
                raise L.GdlError("UnimodalTrainer.step: pe_eps given, but the model has no probabilistic-embedding stacks")
            eps = self.dul.check_eps(pe_eps[0 if self.modality == "audio" else 1])
        self._bind()
        caller = torch.cuda.current_stream(self.device)
        main, lane = self.chain, self.lane
        self.eng.borrow_side_stream(lane.cuda_stream)
        main.wait_stream(caller)
        with torch.cuda.stream(main):
            label = label.contiguous()
            B, n, st = self.B, self.n_classes, main.cuda_stream
            self._mark(main, "start")
            if self.pe:
                _, fmap = self.eng.forward(x, True, want_feat=False, want_fmap=True)
                self.dul.forward(fmap, self.f, self.seed, self.steps, eps)
            else:
                self.eng.forward(x, True, feat_out=self.f)
            self._diversity(self.eng, 0)
            self._mark(main, "fwd_done")
            L.call("gdl_head_cls_ce", L.ptr(self.f), L.ptr(self.pviews[0]), L.ptr(self.pviews[1]), L.ptr(label), 1.0,
                   L.ptr(self.out), L.ptr(self.losses), L.ptr(self.dlogits), L.ptr(self.df), B, n, 512, st)
            self._mark(main, "head_done")
            ev = main.record_event()
            # the classifier's own gradients need only dlogits and the features: on the lane, beside the encoder backward
            lane.wait_event(ev)
            with torch.cuda.stream(lane):
                L.call("gdl_head_cls_bwd", L.ptr(self.f), L.ptr(self.pviews[0]), L.ptr(self.dlogits), None, L.ptr(self.gviews[0]),
                       L.ptr(self.gviews[1]), B, n, 512, lane.cuda_stream)
                ev_cls = lane.record_event()
            if self.pe:
                self.eng.backward(self.gviews[2:62], dfmap=self.dul.backward(self.df, self.beta, self.seed, self.steps, eps))
            else:
                self.eng.backward(self.gviews[2:], dfeat=self.df)
            main.wait_event(ev_cls)
            self._finish_step(main, st)
        caller.wait_stream(main)

    # ------------------------------------------------------------------ validation (main.py's valid())
    def valid(self, batches, bank=None):
        """Eval-mode forward (BatchNorm running statistics) of every (spec, image, label) batch, arg-max of `out` and the
        per-class counters on the device, one host copy at the end.  The reference's valid() counts its three (identical) logit
        sets: returns (acc, acc, acc); `valid_counts` rows = num, acc, acc, acc per class.
        bank: a gdl.ScoreBank of sets = 1 that every batch is appended to behind its counters (mAP / top-k / confusion from
        `bank.report()`), refused before the first launch if it does not fit; nothing else changes."""
        n = self.n_classes
        if bank is not None:
            batches = list(batches)
            bank.check(n, 1, self.device, sum(int(b[2].shape[0]) for b in batches), "UnimodalTrainer.valid")
        cnt = torch.zeros((2, n), dtype=torch.int64, device=self.device)
        for spec, image, label in batches:
            x = self._input(spec, image)
            self._prepare(x)
            self._check_label(label)
            self._bind()
            label = label.contiguous()
            st = L.cur_stream()
            if self.pe:
                self.eng.forward(x, False, feat_out=self.f_raw)
                self.dul.eval(self.f_raw, self.f)
            else:
                self.eng.forward(x, False, feat_out=self.f)
            L.call("gdl_head_cls_fwd", L.ptr(self.f), L.ptr(self.pviews[0]), L.ptr(self.pviews[1]), L.ptr(self.out), self.B, n,
                   512, st)
            L.call("gdl_eval_count", L.ptr(self.out), None, None, L.ptr(label), self.B, n, cnt[0].data_ptr(), cnt[1].data_ptr(),
                   None, None, st)
            if bank is not None:
                bank.append(self.out, None, None, label, stream=st)
        c = cnt.cpu().numpy().astype("float64")
        self.valid_counts = c[[0, 1, 1, 1]]
        acc = c[1].sum() / max(c[0].sum(), 1.0)
        return acc, acc, acc

    # ------------------------------------------------------------------ results (host sync)
    def read(self):
        """Synchronises and returns the quantities the reference prints / logs per step (its three losses are one)."""
        r = self._read_stats((self.eng,))
        loss = float(self.losses.cpu().numpy()[0])
        r.update(loss_f=loss, loss_a=loss, loss_v=loss, out=self.out.cpu().numpy())
        if self.pe:
            r["regurize_a" if self.modality == "audio" else "regurize_v"] = float(self.dul.reg.cpu().numpy()[0])
        return self._read_diversity(r)
