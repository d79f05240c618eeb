"""Drop-in mirror of /root/reference/models/basic_model.py (`AVClassifier_DGL`, :10-86).

Same constructor (reads args.fusion_method / dataset / modality), same attribute and parameter
names in the same registration order (fusion head, audio_net, visual_net), same forward
signature and return order `(out, a_out, v_out)`.  The two encoders run concurrently on two
HIP streams.  All four DGL fusion heads of the reference are built (`concat`, `sum`, `gated` with
x_gate=True, `film`; fusion_modules.py:16-30,45-59,126-178,213-250) for the full-modality setting of the
DGL scripts.  `modality` 'audio' / 'visual' builds the unimodal baselines of basic_model.py:46-59, 88-122 (one encoder and a
`Linear(512, n_classes)` classifier, csrc/head_cls.hip; the fusion head is still constructed, as in the reference, so that
its checkpoints load with strict=True); any other value raises NotImplementedError.  FiLM_DGL handles at most 512 samples per
call (its kernels walk groups of 64 samples, one sample per lane of a wavefront; workspace 0.47 GiB at 64, 3.5 GiB at 512).
"""
import torch
import torch.nn as nn

from gdl import _lib as L

from .backbone import resnet18
from .fusion_modules import (ConcatFusion, ConcatFusion_DGL, FiLM, FiLM_DGL, GatedFusion, GatedFusion_DGL,  # noqa: F401
                             SumFusion, SumFusion_DGL)

N_CLASSES = {'VGGSound': 309, 'KineticSound': 34, 'kinect400': 400, 'CREMAD': 6, 'AVE': 28}  # basic_model.py:15-26


class _ClassifierFn(torch.autograd.Function):
    """out = f W^T + b and its autograd over gdl_head_cls_fwd / gdl_head_cls_bwd (csrc/head_cls.hip)."""

    @staticmethod
    def forward(ctx, f, W, b):
        if not (f.is_cuda and W.is_cuda and b.is_cuda):
            raise RuntimeError("gdl: the classifier runs on the GPU only; move the module and its inputs to the device")
        f, W, b = f.float().contiguous(), W.float().contiguous(), b.float().contiguous()
        if f.dim() != 2 or f.shape[1] != W.shape[1]:
            raise RuntimeError(f"gdl: the classifier takes [B, {W.shape[1]}] features, got {tuple(f.shape)}")
        B, n = f.shape[0], W.shape[0]
        out = torch.empty((B, n), device=f.device)
        L.call("gdl_head_cls_fwd", L.ptr(f), L.ptr(W), L.ptr(b), L.ptr(out), B, n, W.shape[1], L.cur_stream())
        ctx.save_for_backward(f, W)
        return out

    @staticmethod
    def backward(ctx, g_out):
        f, W = ctx.saved_tensors
        B, n = f.shape[0], W.shape[0]
        go = g_out.float().contiguous()
        df = torch.empty_like(f) if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(W) if ctx.needs_input_grad[1] else None
        db = torch.empty(n, device=f.device) if ctx.needs_input_grad[2] else None
        L.call("gdl_head_cls_bwd", L.ptr(f), L.ptr(W), L.ptr(go), L.ptr(df), L.ptr(dW), L.ptr(db), B, n, W.shape[1],
               L.cur_stream())
        return df, dW, db


class Classifier(nn.Linear):
    """The `nn.Linear(512, n_classes)` of the unimodal baselines (basic_model.py:49,56): nn.Linear's constructor, parameter
    names and initialisation; forward and backward are the library's kernels."""

    def forward(self, f):
        return _ClassifierFn.apply(f, self.weight, self.bias)


class AVClassifier_DGL(nn.Module):
    def __init__(self, args):
        super(AVClassifier_DGL, self).__init__()
        fusion = args.fusion_method
        if args.dataset not in N_CLASSES:
            raise NotImplementedError('Incorrect dataset name {}'.format(args.dataset))
        n_classes = N_CLASSES[args.dataset]
        if fusion == 'sum':
            self.fusion_module = SumFusion_DGL(output_dim=n_classes)
        elif fusion == 'concat':
            self.fusion_module = ConcatFusion_DGL(output_dim=n_classes)
        elif fusion == 'gated':
            self.fusion_module = GatedFusion_DGL(output_dim=n_classes, x_gate=True)
        elif fusion == 'film':
            self.fusion_module = FiLM_DGL(output_dim=n_classes, x_film=True)
        else:
            raise NotImplementedError('Incorrect fusion method: {}!'.format(fusion))
        if args.modality not in ('full', 'audio', 'visual'):
            raise NotImplementedError("gdl: modality must be 'full', 'audio' or 'visual', got {!r}".format(args.modality))
        # registration order of basic_model.py:42-59
        if args.modality == 'full':
            self.audio_net = resnet18(modality='audio', args=args)
            self.visual_net = resnet18(modality='visual', args=args)
        elif args.modality == 'visual':
            self.visual_net = resnet18(modality='visual', args=args)
            self.visual_classifier = Classifier(512, n_classes)
        else:
            self.audio_net = resnet18(modality='audio', args=args)
            self.audio_classifier = Classifier(512, n_classes)
        self.modality = args.modality
        self.args = args
        self._side = None

    def _forward_unimodal(self, audio, visual):
        """basic_model.py:88-122: the one encoder, its pooling, the classifier; the same logits three times.  The other
        modality's input is ignored."""
        if self.modality == 'audio':
            if not audio.is_cuda:
                raise RuntimeError("gdl: the model runs on the GPU only; move it and its inputs to the device")
            out = self.audio_classifier(self.audio_net.forward_pooled(audio))
            return out, out, out
        if not visual.is_cuda:
            raise RuntimeError("gdl: the model runs on the GPU only; move it and its inputs to the device")
        if visual.dim() != 5:
            raise RuntimeError("gdl: visual input must be [B,3,T,H,W] (backbone.py:162)")
        # the reference regroups the B*T frame maps by args.batch_size, not by the input's own batch (:94-95)
        Bx, C, T, H, W = visual.shape
        B = int(self.args.batch_size)
        if B <= 0 or (Bx * T) % B:
            raise RuntimeError(f"gdl: {Bx * T} frames ({Bx} x {T}) do not divide into args.batch_size = {B} samples "
                               "(basic_model.py:94-95 views the frame maps as [batch_size, -1, C, H, W])")
        if B != Bx:  # frames in (b, t) order, cut into B runs of Bx*T/B (a copy: layout only)
            visual = visual.permute(0, 2, 1, 3, 4).reshape(B, Bx * T // B, C, H, W).permute(0, 2, 1, 3, 4).contiguous()
        out = self.visual_classifier(self.visual_net.forward_pooled(visual))
        return out, out, out

    def forward(self, audio, visual):
        if self.modality != 'full':
            return self._forward_unimodal(audio, visual)
        cur = torch.cuda.current_stream(audio.device)
        if self._side is None or self._side.device != audio.device:
            self._side = torch.cuda.Stream(device=audio.device)
        side = self._side
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            a = self.audio_net.forward_pooled(audio)  # [B,512]
        v = self.visual_net.forward_pooled(visual)  # [B,512]
        cur.wait_stream(side)
        a.record_stream(cur)
        a_out, v_out, out = self.fusion_module(a, v)
        return out, a_out, v_out


class AVClassifier_DGL_Swin(nn.Module):
    """BASELINE config 5: DGL with a Swin visual branch.  NOT a class of the reference -- its `main_dgl.py:236-240`
    refuses every backbone but `resnet`, and `models/basic_model.py:7` only imports `SwinTransformer` -- but
    the composition SURVEY row N4 defines from the reference's own parts: the ResNet18 audio encoder and its pooling
    (basic_model.py:65-75), `SwinTransformer` with Swin-T's settings on the frames (swin_transformer.py:486-674, pooled
    [B*T, 768] features, averaged over the T frames of a sample as `adaptive_avg_pool3d` does for the ResNet branch,
    basic_model.py:77-80), and `ConcatFusion_DGL` over the 512 + 768 features (fusion_modules.py:45-59; the width of
    `ConcatFusion_Swin`, :79-88, with the audio branch at 512).  Returns (out, a_out, v_out) like `AVClassifier_DGL`."""

    SWIN_T = dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, drop_path_rate=0.)

    def __init__(self, args, swin_kwargs=None):
        super(AVClassifier_DGL_Swin, self).__init__()
        from .swin_transformer import SwinTransformer

        if args.dataset not in N_CLASSES:
            raise NotImplementedError('Incorrect dataset name {}'.format(args.dataset))
        if args.fusion_method != 'concat':
            raise NotImplementedError('gdl: the Swin composition is built with the concat DGL head only')
        kw = dict(self.SWIN_T if swin_kwargs is None else swin_kwargs)
        feat = kw["embed_dim"] * 2 ** (len(kw["depths"]) - 1)
        self.fusion_module = ConcatFusion_DGL(input_dim=512 + feat, output_dim=N_CLASSES[args.dataset])
        self.audio_net = resnet18(modality='audio', args=args)
        self.visual_net = SwinTransformer(args, 'visual', **kw)
        self.modality = 'full'
        self.args = args

    def forward(self, audio, visual):
        a = self.audio_net.forward_pooled(audio)  # [B, 512]
        v = self.visual_net.forward_pooled(visual)  # [B, 768]
        a_out, v_out, out = self.fusion_module(a, v)
        return out, a_out, v_out


class AVClassifier(nn.Module):
    """BASELINE config 1: the jointly trained (non-DGL) model of main.py.  The reference class of this name
    no longer exists in models/basic_model.py (main.py:19 cannot be imported); this
    restates its math from the parts that do exist: the two encoders, the pooling glue of
    basic_model.py:73-82 and the joint fusion heads `ConcatFusion` (fusion_modules.py:33-42), `SumFusion` (:5-13),
    `GatedFusion(x_gate=True)` (:181-210) and `FiLM(dim=512)` (:91-124), chosen by args.fusion_method as
    AVClassifier_DGL chooses their DGL twins.  Returns the head's tuple (a, v, out)."""

    def __init__(self, args):
        super(AVClassifier, self).__init__()
        if args.dataset not in N_CLASSES:
            raise NotImplementedError('Incorrect dataset name {}'.format(args.dataset))
        fusion, n_classes = args.fusion_method, N_CLASSES[args.dataset]
        if fusion == 'sum':
            self.fusion_module = SumFusion(output_dim=n_classes)
        elif fusion == 'concat':
            self.fusion_module = ConcatFusion(output_dim=n_classes)
        elif fusion == 'gated':
            self.fusion_module = GatedFusion(output_dim=n_classes, x_gate=True)
        elif fusion == 'film':
            self.fusion_module = FiLM(dim=512, output_dim=n_classes, x_film=True)
        else:
            raise NotImplementedError('Incorrect fusion method: {}!'.format(fusion))
        self.audio_net = resnet18(modality='audio', args=args)
        self.visual_net = resnet18(modality='visual', args=args)
        self.modality = 'full'
        self.args = args

    def forward(self, audio, visual):
        a = self.audio_net.forward_pooled(audio)
        v = self.visual_net.forward_pooled(visual)
        a, v, out = self.fusion_module(a, v)
        return a, v, out


class AVClassifier_MLA(nn.Module):
    """The model of alternating unimodal training on a shared head (MLA, Zhang et al., CVPR 2024): the two
    ResNet18 encoders as `AVClassifier_DGL` builds them and ONE `Linear(512, n_classes)` that classifies either modality's pooled
    feature.  NOT a class of the reference (it has no MLA script): a parameter container over its parts for `gdl.MLATrainer`,
    registered as audio_net, visual_net, classifier.  forward returns (out, out_a, out_v) with the static fusion out = 0.5 out_a
    + 0.5 out_v; the entropy-weighted fusion is `MLATrainer.valid(dynamic=True)` / `gdl_mla_fuse`."""

    def __init__(self, args):
        super(AVClassifier_MLA, self).__init__()
        if args.dataset not in N_CLASSES:
            raise NotImplementedError('Incorrect dataset name {}'.format(args.dataset))
        self.audio_net = resnet18(modality='audio', args=args)
        self.visual_net = resnet18(modality='visual', args=args)
        self.classifier = Classifier(512, N_CLASSES[args.dataset])
        self.modality = 'full'
        self.args = args

    def forward(self, audio, visual):
        out_a = self.classifier(self.audio_net.forward_pooled(audio))
        out_v = self.classifier(self.visual_net.forward_pooled(visual))
        return 0.5 * out_a + 0.5 * out_v, out_a, out_v
