"""The probabilistic-embedding branch of main.py (`--pe 1 --beta b`) as a per-encoder stage of the native runners.

The stage sits wholly between an encoder engine's final map and the pooled feature the heads see, so it is head-independent:
  forward   behind the engine's training forward, on that encoder's stream: the engine's final map (its float32 NCHW output,
            back in the storage dtype and layout through gdl_nchw_f32_to_nhwc: exact, the map was rounded when it was stored),
            the two 1x1 weights packed in the storage dtype (as the engine packs its own convolutions, every step),
            z = x W^T + b for both stacks (gdl_conv_fwd_bias), each stack's train-mode BatchNorm statistics (gdl_bn_stats, gdl_bn_finalize_train: the running
            statistics of the modules' buffers are updated there), and gdl_dul_sample -> the pooled feature f and `regurize`
  backward  between the launch that produces the encoder's feature gradient and the engine's backward, on the same chain:
            gdl_dul_bwd_reduce, gdl_bn_bwd_finalize of each stack (dgamma / dbeta straight into the gradient arena),
            gdl_dul_bwd_apply, the two data gradients (the second adds the first), handed to the engine's backward as its
            float32 NCHW map gradient (gdl_nhwc_to_nchw_f32), and the two weight gradients into the arena
  eval      gdl_dul_eval on the engine's pooled feature with the mu stack's running statistics
The noise is never stored: forward and backward regenerate it from (seed, step count, modality), or read the caller's map.
include/gdl_hip.h states the arithmetic; csrc/dul.hip the kernels' fixed orders.  The convolution biases get no gradient launch:
their gradient is exactly 0 (a bias in front of a train-mode BatchNorm) and their arena slots stay at the zeros they were made with.
"""
import torch

from . import _lib as L

N_DUL = 8  # tensors the branch adds to an encoder: (conv weight, conv bias, BatchNorm weight, BatchNorm bias) x (mu, logvar)


def has_stacks(net):
    """whether a module carries the two stacks (models.backbone.resnet18 with args.pe)"""
    return bool(getattr(net, "pe", False)) and hasattr(net, "mu_dul_backbone") and hasattr(net, "logvar_dul_backbone")


class DulStage:
    def __init__(self, net, eng, pviews, gviews):
        """net: the encoder module (its two BatchNorms' buffers are updated in place); eng: its EncoderEngine; pviews / gviews: the
        8 parameter / gradient arena views in registration order."""
        if len(pviews) != N_DUL or len(gviews) != N_DUL:
            raise L.GdlError("DulStage: the branch has 8 tensors per encoder")
        lib = self.lib = L.load()
        self.eng, self.dt, self.device = eng, eng.dtype, eng.device
        self.modality = eng.modality
        self.n_img, _, self.h, self.w = eng.out_shape
        self.P = self.h * self.w
        self.B, self.T = eng.shape[0], eng.shape[1]
        M = self.M = self.n_img * self.P
        self.pv, self.gv = list(pviews), list(gviews)
        self.bns = (net.mu_dul_backbone[1], net.logvar_dul_backbone[1])
        d, td = self.device, L.torch_dtype(self.dt)
        with torch.cuda.device(d):
            self.x = torch.empty((M, 512), dtype=td, device=d)   # the final map, NHWC in the storage dtype
            self.dx = torch.empty((M, 512), dtype=td, device=d)  # its gradient
            self.dx_nchw = torch.empty(eng.out_shape, device=d)  # ... as the engine's backward takes it
            self.z = torch.empty((2, M, 512), dtype=td, device=d)
            self.dz = torch.empty((2, M, 512), dtype=td, device=d)
            self.w_krsc = torch.empty((2, 512, 512), dtype=td, device=d)
            self.w_crsk = torch.empty((2, 512, 512), dtype=td, device=d)
            self.bn = torch.zeros((2, 4, 512), device=d)  # per stack: scale, shift, save_mean, save_rstd
            self.coef = torch.empty((2, 2, 512), device=d)
            self.eval_ss = torch.empty((2, 512), device=d)
            self.tiles = lib.gdl_bn_stats_tiles(M)
            self.part = torch.empty((2, self.tiles, 512, 2), device=d)
            self.blocks = lib.gdl_bn_bwd_blocks(M, 512)
            self.bpart = torch.empty((2, self.blocks, 512, 2), device=d)
            self.tab = {}
            for mode in (L.GATHER_FWD, L.GATHER_DGRAD):
                t = torch.empty(lib.gdl_conv_table_bytes(mode, M, 1, 1, 1, 1, 1, 0), dtype=torch.uint8, device=d)
                L.call("gdl_conv_build_table", mode, self.dt, M, 1, 1, 512, 512, 1, 1, 1, 0, L.ptr(t), L.cur_stream())
                self.tab[mode] = t
            self.wg_ws = torch.empty(max(lib.gdl_conv_wgrad_workspace_bytes(self.dt, M, 1, 1, 512, 512, 1, 1, 1, 0), 16),
                                     dtype=torch.uint8, device=d)
            # gdl_dul_sample's ticket counter: zeroed here once, handed back at zero by every launch
            self.ws = torch.zeros(lib.gdl_dul_sample_workspace_bytes(self.dt, self.n_img, self.T), dtype=torch.uint8, device=d)
            self.reg = torch.zeros(1, device=d)

    def check_eps(self, eps):
        """a caller-supplied noise map: float32 [M][512] ([n_img][P][512] order), contiguous, on the device"""
        if eps is None:
            return None
        if not torch.is_tensor(eps) or eps.dtype != torch.float32 or eps.numel() != self.M * 512 or not eps.is_contiguous() or \
                eps.device != self.device:
            raise L.GdlError(f"pe_eps: each map must be a contiguous float32 [{self.M}, 512] tensor on {self.device} "
                             "(rows in [n_img][P] order)")
        return eps

    def forward(self, fmap, f, seed, step, eps=None):
        """behind `_, fmap = eng.forward(x, True, want_feat=False, want_fmap=True)` on the current stream: f [B][512], self.reg"""
        st, dt, M, pv = L.cur_stream(), self.dt, self.M, self.pv
        L.call("gdl_nchw_f32_to_nhwc", dt, L.ptr(fmap), L.ptr(self.x), self.n_img, self.h, self.w, 512, st)
        for i in range(2):
            L.call("gdl_pack_weight", dt, L.ptr(pv[4 * i]), L.ptr(self.w_krsc[i]), L.ptr(self.w_crsk[i]), 512, 512, 1, 1, st)
        for i in range(2):
            L.call("gdl_conv_fwd_bias", dt, L.ptr(self.x), L.ptr(self.w_krsc[i]), L.ptr(self.z[i]), L.ptr(pv[4 * i + 1]), None, None,
                   L.ptr(self.tab[L.GATHER_FWD]), M, 1, 1, 512, 512, 1, 1, 1, 0, st)
        for i, bn in enumerate(self.bns):
            L.call("gdl_bn_stats", dt, L.ptr(self.z[i]), L.ptr(self.part[i]), M, 512, st)
            b = self.bn[i]
            L.call("gdl_bn_finalize_train", L.ptr(self.part[i]), self.tiles, 512, float(M), L.ptr(pv[4 * i + 2]), L.ptr(pv[4 * i + 3]),
                   1e-5, 0.1, L.ptr(bn.running_mean), L.ptr(bn.running_var), L.ptr(bn.num_batches_tracked), L.ptr(b[2]), L.ptr(b[3]),
                   L.ptr(b[0]), L.ptr(b[1]), st)
        L.call("gdl_dul_sample", dt, L.ptr(self.z[0]), L.ptr(self.z[1]), L.ptr(self.bn[0]), L.ptr(self.bn[1]), L.ptr(eps), seed, step,
               self.modality, L.ptr(f), L.ptr(self.reg), None, None, None, None, self.n_img, self.T, self.P, 512, L.ptr(self.ws),
               self.ws.numel(), st)
        self._keep = (eps, fmap)

    def backward(self, df, beta, seed, step, eps=None):
        """from the head's df [B][512] on the current stream: the 6 non-zero parameter gradients into the arena; returns the
        gradient w.r.t. the post-ReLU map, float32 NCHW, for eng.backward(grads, dfmap=...) on the same stream"""
        st, dt, M, gv = L.cur_stream(), self.dt, self.M, self.gv
        n, T, P = self.n_img, self.T, self.P
        L.call("gdl_dul_bwd_reduce", dt, L.ptr(self.z[0]), L.ptr(self.z[1]), L.ptr(df), L.ptr(eps), seed, step, self.modality, beta,
               L.ptr(self.bn[0]), L.ptr(self.bn[1]), L.ptr(self.bpart[0]), L.ptr(self.bpart[1]), n, T, P, 512, st)
        for i in range(2):
            L.call("gdl_bn_bwd_finalize", L.ptr(self.bpart[i]), self.blocks, 512, float(M), L.ptr(gv[4 * i + 2]), L.ptr(gv[4 * i + 3]),
                   L.ptr(self.coef[i]), st)
        L.call("gdl_dul_bwd_apply", dt, L.ptr(self.z[0]), L.ptr(self.z[1]), L.ptr(df), L.ptr(eps), seed, step, self.modality, beta,
               L.ptr(self.bn[0]), L.ptr(self.bn[1]), L.ptr(self.pv[2]), L.ptr(self.pv[6]), L.ptr(self.coef[0]), L.ptr(self.coef[1]),
               L.ptr(self.dz[0]), L.ptr(self.dz[1]), n, T, P, 512, st)
        tab = L.ptr(self.tab[L.GATHER_DGRAD])
        L.call("gdl_conv_dgrad", dt, L.ptr(self.dz[0]), L.ptr(self.w_crsk[0]), L.ptr(self.dx), None, tab, M, 1, 1, 512, 512, 1, 1, 1, 0, st)
        L.call("gdl_conv_dgrad", dt, L.ptr(self.dz[1]), L.ptr(self.w_crsk[1]), L.ptr(self.dx), L.ptr(self.dx), tab, M, 1, 1, 512, 512, 1, 1, 1, 0, st)
        for i in range(2):
            L.call("gdl_conv_wgrad", dt, L.ptr(self.dz[i]), L.ptr(self.x), L.ptr(gv[4 * i]), L.ptr(self.tab[L.GATHER_FWD]), M, 1, 1, 512, 512,
                   1, 1, 1, 0, L.ptr(self.wg_ws), self.wg_ws.numel(), st)
        L.call("gdl_nhwc_to_nchw_f32", dt, L.ptr(self.dx), L.ptr(self.dx_nchw), self.n_img, self.h, self.w, 512, st)
        self._keep_b = (df, eps)
        return self.dx_nchw

    def eval(self, f_in, f_out):
        """valid(): f_out = BN_eval(W_mu f_in + b_mu) on the engine's pooled feature (the logvar stack is not evaluated)"""
        st, pv, bn = L.cur_stream(), self.pv, self.bns[0]
        L.call("gdl_bn_finalize_eval", 512, L.ptr(pv[2]), L.ptr(pv[3]), 1e-5, L.ptr(bn.running_mean), L.ptr(bn.running_var),
               L.ptr(self.eval_ss[0]), L.ptr(self.eval_ss[1]), st)
        L.call("gdl_dul_eval", L.ptr(f_in), L.ptr(pv[0]), L.ptr(pv[1]), L.ptr(self.eval_ss[0]), L.ptr(self.eval_ss[1]), L.ptr(f_out),
               f_in.shape[0], 512, st)
