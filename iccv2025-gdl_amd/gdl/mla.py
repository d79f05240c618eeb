"""Native runner of alternating unimodal training on a shared head (MLA: "Multimodal Representation Learning by Alternating
Unimodal Adaptation", Zhang et al., CVPR 2024) -- DESIGN.md section 8 is this project's statement of the method.

One `step(spec, image, label)` is two unimodal half-steps in fixed order, audio then visual, each main.py's unimodal step
(gdl.unimodal) on ONE shared `Linear(512, n)`: the encoder's training forward, gdl_head_cls_ce, the encoder's backward,
gdl_head_cls_bwd for the head's dW / db, clip_grad_norm_(40) and SGD over THIS half-step's tensors only (the head and one
encoder; the other encoder's parameters and momentum are not touched, torch's zero_grad(set_to_none=True) behaviour).  With
`shaping` the head's dW is multiplied by a projector P [512][512] that is updated recursively against the mean feature of the
PREVIOUS half-step (csrc/mla.hip); at test time the two unimodal logit sets are fused by entropy weights (gdl_mla_fuse).

One arena [audio 60 | classifier 2 | visual 60] with the optimizer groups 1 / 0 / 2, and TWO gdl_optim descriptors over the
overlapping contiguous sub-ranges [audio | classifier] and [classifier | visual]: a half-step's statistics, clip and update are
the existing kernels on its own range.  optim.hip takes float4 accesses from the base it is given, so the second range must
start on a 16-byte boundary: the audio encoder's element count is a multiple of 4 (checked at construction).

Streams of one step (A, V = the process-wide chain streams, C = the stream step() is called on, idle for the step's duration):
  V: the visual training forward, from the start of the step -- it does not depend on the head -- beside the audio half-step
  C: [projector update against r_prev]                                           (shaping; off the chain)
  A: audio forward -> gdl_head_cls_ce -> audio backward (weight gradients on C) -> statistics -> clip + update -> event U
  C: behind the head: gdl_head_cls_bwd -> [gdl_mla_project] -> gdl_mla_feature_mean (r_prev <- r_a), then the audio weight
     gradients, then [the visual half-step's projector update against r_a]
  V: waits for U (W, b and the head's gradient buffers are free) -> gdl_head_cls_ce -> visual backward (weight gradients on
     the engine's side stream) -> statistics -> clip + update
  A: idle after U: the visual half-step's gdl_head_cls_bwd -> [gdl_mla_project];   C: gdl_mla_feature_mean (r_prev <- r_v)
Only gdl_mla_project stands between gdl_head_cls_bwd and the statistics.  Nothing is read back unless `read()` is called.
"""
import torch

from . import _lib as L
from .encoder import EncoderEngine
from .trainer import ArenaTrainer


def mla_alpha(step_in_epoch, steps_per_epoch):
    """The shaping constant's schedule, in the style of `gdl.multistep_lr`: 0.1 ** (1 + step_in_epoch / steps_per_epoch) --
    0.1 at the start of an epoch, falling to 0.01 at its end.  Assign it to `trainer.shaping_alpha` before a step."""
    if steps_per_epoch <= 0:
        raise ValueError(f"mla_alpha: steps_per_epoch must be positive, got {steps_per_epoch!r}")
    return 0.1 ** (1.0 + step_in_epoch / steps_per_epoch)


class MLATrainer(ArenaTrainer):
    """The arenas, the momentum arena and its checkpoint and `grad(name)` are ArenaTrainer's; here: the 122-tensor list, the two
    descriptors, the two half-steps, the projector's state, valid() with the entropy-weighted fusion, and read()."""

    _script = "main.py"
    HALVES = ("audio", "visual")

    def __init__(self, model, lr, momentum=0.9, weight_decay=None, max_norm=40.0, dtype=None, shaping=True, shaping_alpha=0.1,
                 normalize=True, *, optimizer="sgd", process_group=None, journal=0, diversity=False, modulation="Normal",
                 prototypes=None):
        """shaping: multiply the head's weight gradient by the projector (off: two plain unimodal half-steps on the shared
        head).  shaping_alpha: the constant alpha_s > 0 of the projector update, a plain attribute the caller may set per step
        (`gdl.mla_alpha`), passed as a kernel argument.  normalize: P <- P / ||P||_F after every update.
        The keyword-only arguments exist to be refused: none of them is built on this runner."""
        who = "MLATrainer"
        if optimizer != "sgd":
            raise L.GdlError(f"{who}: only optimizer='sgd' is built (got {optimizer!r}): the library's Adam / AdaGrad updates take "
                             "one step count per descriptor, which cannot describe a head that steps twice per batch")
        if process_group is not None:
            raise L.GdlError(f"{who}: data-parallel runs (process_group) are not built for alternating training")
        for key, val, off in (("journal", journal, 0), ("diversity", diversity, False), ("modulation", modulation, "Normal"),
                              ("prototypes", prototypes, None)):
            if val is not off and val != off:
                raise L.GdlError(f"{who}: {key}={val!r} is not built on this runner (DGLTrainer / UnimodalTrainer carry it)")
        if type(model).__name__ != "AVClassifier_MLA":
            raise L.GdlError(f"{who}: the model must be models.basic_model.AVClassifier_MLA, got {type(model).__name__}")
        cls = model.classifier
        device = cls.weight.device
        if device.type != "cuda":
            raise L.GdlError(f"{who}: the model must live on an MI355X (cuda) device; there is no CPU path")
        for net in (model.audio_net, model.visual_net):
            if hasattr(net, "cfg") and hasattr(net, "num_features"):
                raise L.GdlError(f"{who}: the Swin branch is not built for alternating training (ResNet18 encoders only)")
        if tuple(cls.weight.shape[1:]) != (512,) or cls.weight.shape[0] > 512:
            raise L.GdlError(f"{who}: the classifier must be Linear(512, n_classes <= 512)")
        self.model = model
        self.mode = "mla"
        self.dtype = dtype if dtype is not None else model.audio_net.gdl_dtype
        self.n_classes = cls.weight.shape[0]
        self.shaping, self.normalize = bool(shaping), bool(normalize)
        self.shaping_alpha = shaping_alpha
        self._check_alpha()
        if getattr(model.audio_net, "pe", False) or getattr(model.visual_net, "pe", False):
            raise L.GdlError(f"{who}: the probabilistic-embedding branch (args.pe) is not built for alternating unimodal training")
        named = [("audio_net." + n, p) for n, p in model.audio_net.named_parameters()]
        named += [("classifier.weight", cls.weight), ("classifier.bias", cls.bias)]
        named += [("visual_net." + n, p) for n, p in model.visual_net.named_parameters()]
        if len(named) != 122:
            raise L.GdlError(f"{who}: both encoders must be the ResNet18 mirror (60 tensors each)")
        super().__init__(named, [1] * 60 + [0, 0] + [2] * 60, device, "sgd", lr, momentum, weight_decay, max_norm)
        self.losses = torch.zeros(2, device=device)  # loss_a, loss_v
        # the projector's state, beside the model: P = I, no previous feature mean
        self.P = torch.eye(512, device=device)
        self.r_prev = torch.zeros(512, device=device)
        self.have_prev = 0
        self.proj_ws_bytes = self.lib.gdl_mla_projector_workspace_bytes()
        self.proj_ws = torch.empty(self.proj_ws_bytes, dtype=torch.uint8, device=device)
        self.eng = None

    # ------------------------------------------------------------------ the two descriptors
    def _create_descriptors(self, offs, group):
        """[audio | classifier] = segments 0 .. 61, [classifier | visual] = segments 60 .. 121; each descriptor's offsets count
        from its own base, which the update's float4 accesses need on a 16-byte boundary."""
        self.opt = None  # (ArenaTrainer.close: no whole-arena descriptor)
        self.half = {}
        for m, lo, hi in (("audio", 0, 62), ("visual", 60, 122)):
            if offs[lo] % 4:
                raise L.GdlError(f"MLATrainer: the {m} half-step's range starts at element {offs[lo]} of the arena, not on a "
                                 "16-byte boundary (the optimizer kernels take float4 accesses from their base)")
            h, nb, ws, stats = self._descriptor([o - offs[lo] for o in offs[lo:hi + 1]], group[lo:hi])
            self.half[m] = dict(opt=h, ws=ws, ws_bytes=nb, stats=stats, lo=lo, hi=hi, base=4 * offs[lo])

    def close(self):
        """Releases both optimizer descriptors.  Idempotent; also run by __del__."""
        for d in getattr(self, "half", {}).values():
            if d["opt"]:
                self.lib.gdl_optim_destroy(d["opt"])
                d["opt"] = None

    def _check_alpha(self):
        a = self.shaping_alpha
        if self.shaping and not (isinstance(a, (int, float)) and 0.0 < float(a) < float("inf")):
            raise L.GdlError(f"MLATrainer: shaping_alpha must be a finite positive float, got {a!r}")

    # ------------------------------------------------------------------ setup per batch shape
    def _prepare(self, spec, image):
        for x, dim, want in ((spec, 3, "spec [B,F,T']"), (image, 5, "image [B,3,T,H,W]")):
            if x is None or x.dim() != dim or (dim == 5 and x.shape[1] != 3):
                raise L.GdlError(f"MLATrainer: the model takes {want}")
            if x.device != self.device:
                raise L.GdlError(f"MLATrainer: the inputs must be on {self.device}, got {x.device} (there is no CPU path)")
        if spec.shape[0] != image.shape[0]:
            raise L.GdlError("MLATrainer: spec and image must hold the same number of samples")
        key = tuple(spec.shape) + tuple(image.shape)
        if getattr(self, "_key", None) == key:
            return
        self._key = key
        B, n, d = spec.shape[0], self.n_classes, self.device
        self.eng = {"audio": EncoderEngine("audio", self.dtype, B, 1, spec.shape[1], spec.shape[2], d),
                    "visual": EncoderEngine("visual", self.dtype, B, *image.shape[2:], d)}
        self.eng["visual"].side_stream(True)  # the fourth lane, as DGLTrainer: the audio engine's is the caller's stream
        self.f = {m: torch.empty((B, 512), device=d) for m in self.HALVES}
        self.df = {m: torch.empty((B, 512), device=d) for m in self.HALVES}
        self.outs = {m: torch.empty((B, n), device=d) for m in self.HALVES}
        self.dlogits = {m: torch.empty((B, n), device=d) for m in self.HALVES}
        self.out = torch.empty((B, n), device=d)
        self.lam = torch.empty((B, 2), device=d)
        self.B = B

    def _bind(self):
        for m in self.HALVES:
            net = getattr(self.model, m + "_net")
            bns = net._bn_layers()
            self.eng[m].set_params([p.data for p in net.parameters()], [b.running_mean for b in bns],
                                   [b.running_var for b in bns], [b.num_batches_tracked for b in bns])

    # ------------------------------------------------------------------ the step
    def step(self, spec, image, label):
        """spec [B,F,T'] float, image [B,3,T,H,W] float, label [B] int64 -- all resident on the device."""
        self._prepare(spec, image)
        self._check_label(label)
        self._check_alpha()
        self._bind()
        caller = torch.cuda.current_stream(self.device)
        self.eng["audio"].borrow_side_stream(caller.cuda_stream)
        self.s_a.wait_stream(caller)
        self.s_v.wait_stream(caller)
        label = label.contiguous()
        self._mark(self.s_a, "start")
        with torch.cuda.stream(self.s_v):  # beside the whole audio half-step: it reads nothing the audio half-step writes
            self.eng["visual"].forward(image, True, feat_out=self.f["visual"])
        self._half_on("audio", caller, spec.unsqueeze(1), label, forward=True)
        self._mark(self.s_a, "audio_done")
        self._half_on("visual", caller, image, label, forward=False)
        self._mark(self.s_v, "end")
        caller.wait_stream(self.s_a)
        caller.wait_stream(self.s_v)
        self.steps += 1

    def _half_step(self, modality, spec, image, label):
        """ONE half-step alone (the tests' handle on what a half-step touches): `step` is `_half_step("audio", ..)` followed by
        `_half_step("visual", ..)` with the visual forward started early."""
        if modality not in self.HALVES:
            raise L.GdlError(f"MLATrainer: modality must be 'audio' or 'visual', got {modality!r}")
        self._prepare(spec, image)
        self._check_label(label)
        self._check_alpha()
        self._bind()
        caller = torch.cuda.current_stream(self.device)
        self.eng["audio"].borrow_side_stream(caller.cuda_stream)
        self.s_a.wait_stream(caller)
        self.s_v.wait_stream(caller)
        self._half_on(modality, caller, spec.unsqueeze(1) if modality == "audio" else image, label.contiguous(), forward=True)
        caller.wait_stream(self.s_a)
        caller.wait_stream(self.s_v)

    def _half_on(self, m, caller, x, label, forward):
        audio = m == "audio"
        chain = self.s_a if audio else self.s_v
        lane = caller if audio else self.s_a  # where the head's own gradients go: idle while the chain runs the backward
        d, eng, B, n = self.half[m], self.eng[m], self.B, self.n_classes
        f, W, b, gW, gb = self.f[m], self.pviews[60], self.pviews[61], self.gviews[60], self.gviews[61]
        shaped = self.shaping and bool(self.have_prev)
        if shaped:  # needs the previous half-step's mean alone: on the caller's stream, off the chain
            with torch.cuda.stream(caller):
                L.call("gdl_mla_projector_update", L.ptr(self.P), L.ptr(self.r_prev), float(self.shaping_alpha),
                       int(self.normalize), L.ptr(self.proj_ws), self.proj_ws_bytes, caller.cuda_stream)
                ev_p = caller.record_event()
        with torch.cuda.stream(chain):
            if forward:
                eng.forward(x, True, feat_out=f)
            if not audio:  # W, b and the head's gradient buffers are free behind the audio half-step's update
                chain.wait_stream(self.s_a)
            L.call("gdl_head_cls_ce", L.ptr(f), L.ptr(W), L.ptr(b), L.ptr(label), 1.0, L.ptr(self.outs[m]),
                   self.losses.data_ptr() + (0 if audio else 4), L.ptr(self.dlogits[m]), L.ptr(self.df[m]), B, n, 512,
                   chain.cuda_stream)
            ev_h = chain.record_event()
        lane.wait_event(ev_h)
        if shaped and lane is not caller:
            lane.wait_event(ev_p)
        with torch.cuda.stream(lane):
            L.call("gdl_head_cls_bwd", L.ptr(f), L.ptr(W), L.ptr(self.dlogits[m]), None, L.ptr(gW), L.ptr(gb), B, n, 512,
                   lane.cuda_stream)
            if shaped:
                L.call("gdl_mla_project", L.ptr(gW), L.ptr(self.P), n, lane.cuda_stream)
            ev_cls = lane.record_event()
        caller.wait_event(ev_h)
        with torch.cuda.stream(caller):  # behind the projector update that read r_prev: the same stream
            L.call("gdl_mla_feature_mean", L.ptr(f), B, L.ptr(self.r_prev), caller.cuda_stream)
        self.have_prev = 1
        with torch.cuda.stream(chain):
            eng.backward(self.gviews[0:60] if audio else self.gviews[62:122], dfeat=self.df[m])
            chain.wait_event(ev_cls)
            st, o = chain.cuda_stream, d["base"]
            L.call("gdl_optim_grad_stats", d["opt"], self.grads.data_ptr() + o, self.max_norm, 1.0, L.ptr(d["stats"]),
                   L.ptr(d["ws"]), d["ws_bytes"], st)
            L.call("gdl_optim_sgd_step", d["opt"], self.params.data_ptr() + o, self.grads.data_ptr() + o,
                   self.momentum.data_ptr() + o, L.ptr(d["stats"]), 1.0, self.lr, self.mu, self.wd, st)

    # ------------------------------------------------------------------ validation
    def valid(self, batches, bank=None, dynamic=True):
        """Eval-mode forwards of both encoders for every (spec, image, label) batch, the shared head on each feature set
        (gdl_head_cls_fwd twice), the test-time fusion (gdl_mla_fuse: entropy weights, or 0.5 / 0.5 with dynamic=False), arg-max
        and per-class counters on the device, one host copy at the end.  Returns (acc, acc_a, acc_v); `valid_counts` rows = num,
        acc, acc_a, acc_v per class.  bank: a gdl.ScoreBank of sets = 3 that every batch is appended to behind its counters."""
        n = self.n_classes
        if bank is not None:
            batches = list(batches)
            bank.check(n, 3, self.device, sum(int(b[2].shape[0]) for b in batches), "MLATrainer.valid")
        cnt = torch.zeros((4, n), dtype=torch.int64, device=self.device)
        main = torch.cuda.current_stream(self.device)
        W, b = self.pviews[60], self.pviews[61]
        for spec, image, label in batches:
            self._prepare(spec, image)
            self._check_label(label)
            self._bind()
            label = label.contiguous()
            ev = main.record_event()
            self.s_a.wait_event(ev)
            self.s_v.wait_event(ev)
            with torch.cuda.stream(self.s_v):
                self.eng["visual"].forward(image, False, feat_out=self.f["visual"])
            with torch.cuda.stream(self.s_a):
                self.eng["audio"].forward(spec.unsqueeze(1), False, feat_out=self.f["audio"])
            main.wait_stream(self.s_a)
            main.wait_stream(self.s_v)
            st = main.cuda_stream
            oa, ov = self.outs["audio"], self.outs["visual"]
            for m in self.HALVES:
                L.call("gdl_head_cls_fwd", L.ptr(self.f[m]), L.ptr(W), L.ptr(b), L.ptr(self.outs[m]), self.B, n, 512, st)
            L.call("gdl_mla_fuse", L.ptr(oa), L.ptr(ov), self.B, n, int(bool(dynamic)), L.ptr(self.out), L.ptr(self.lam), st)
            L.call("gdl_eval_count", L.ptr(self.out), L.ptr(oa), L.ptr(ov), L.ptr(label), self.B, n, cnt[0].data_ptr(),
                   cnt[1].data_ptr(), cnt[2].data_ptr(), cnt[3].data_ptr(), st)
            if bank is not None:
                bank.append(self.out, oa, ov, label, stream=st)
        c = cnt.cpu().numpy().astype("float64")
        self.valid_counts = c
        tot = max(c[0].sum(), 1.0)
        return c[1].sum() / tot, c[2].sum() / tot, c[3].sum() / tot

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self):
        """ArenaTrainer's (the momentum arena, lr, the step count) plus the projector's state: P, r_prev, have_prev."""
        sd = super().state_dict()
        sd.update(P=self.P.detach().clone(), r_prev=self.r_prev.detach().clone(), have_prev=int(self.have_prev))
        return sd

    def load_state_dict(self, sd):
        for k in ("P", "r_prev", "have_prev"):
            if k not in sd:
                raise L.GdlError(f"MLATrainer.load_state_dict: the checkpoint has no {k!r} (not an MLATrainer's)")
        super().load_state_dict(sd)
        self.P.copy_(sd["P"].to(self.device))
        self.r_prev.copy_(sd["r_prev"].to(self.device))
        self.have_prev = int(sd["have_prev"])

    # ------------------------------------------------------------------ results (host sync)
    def read(self):
        """Synchronises and returns loss_a, loss_v, the two logit sets of the last step, and each half-step's statistics under
        "audio" / "visual": total_norm (of what is applied: dW is shaped before it is measured), clip_coef, audio_grad_sum,
        visual_grad_sum (the absent encoder's reads 0.0), grad_norm and grad_absmean by tensor name."""
        torch.cuda.synchronize(self.device)
        bad = sum(e.bn_overflow() for e in (self.eng or {}).values())
        if bad:
            raise FloatingPointError(f"gdl: the statistics of {bad} BatchNorm layer(s) overflowed in the last training forward "
                                     "(activations of mean magnitude beyond 8192: the run has diverged)")
        ls = self.losses.cpu().numpy()
        r = dict(loss_a=float(ls[0]), loss_v=float(ls[1]), out_a=self.outs["audio"].cpu().numpy(),
                 out_v=self.outs["visual"].cpu().numpy())
        for m, d in self.half.items():
            s = d["stats"].cpu().numpy()
            names = self.names[d["lo"]:d["hi"]]
            k = len(names)
            r[m] = {"total_norm": float(s[0]), "clip_coef": float(s[1]), "audio_grad_sum": float(s[2]),
                    "visual_grad_sum": float(s[3]), "grad_norm": dict(zip(names, s[4:4 + k].tolist())),
                    "grad_absmean": dict(zip(names, s[4 + k:4 + 2 * k].tolist()))}
        return r
