"""Swin visual encoder on libgdl_hip: forward + backward of the function the reference's
`SwinTransformer.forward` computes with `args.pe = 0`, `ape = False`, `patch_norm = True` and every dropout / the
stochastic depth at 0 (/root/reference/models/swin_transformer.py:596-634; block :256-295; window attention :124-157;
patch merging :330-353; patch embedding :478-486).

The host side here only plans buffers and enqueues kernels (PyTorch = device allocator + streams):
  * every nn.Linear and the 4x4/4 patch convolution is a 1x1 convolution of the library -- `gdl_conv_fwd`, `gdl_conv_dgrad`,
    `gdl_conv_wgrad` (MFMA implicit GEMM; weights zero-padded so that every width is a multiple of 64: 96 -> 128 in stage 1,
    a QKV row is three such segments);
  * LayerNorm, bias / GELU / residual, window attention (shift, mask, relative-position bias), patch merging and the final
    token mean are the `gdl_swin_*` kernels of csrc/swin.hip.
Everything saved for the backward is kept (nothing recomputed except the attention probabilities).  Every buffer, gather
table and fold table is made by `SwinEngine.__init__`: the passes are fixed launch sequences that allocate nothing.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib as L


class _PackDesc(ctypes.Structure):  # csrc/swin.hip::SwinPackDesc
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("dstT", ctypes.c_void_p)] + \
        [(n, ctypes.c_int32) for n in ("n", "k", "nseg", "nseg_pad", "kseg", "kseg_pad", "np", "kp", "dt", "blk0")]


assert ctypes.sizeof(_PackDesc) == 64


class _RedDesc(ctypes.Structure):  # csrc/swin.hip::SwinRedDesc
    _fields_ = [("partial", ctypes.c_void_p), ("out", ctypes.c_void_p)] + [(n, ctypes.c_int32) for n in ("rows", "width", "blk0", "stride")]


assert ctypes.sizeof(_RedDesc) == 32


def _ld(c):
    return (c + 63) // 64 * 64


def _knob(name, off):
    """False where the tuning aid `name` is switched off (the value `off`; read only under GDL_TUNING=1)"""
    return not (os.environ.get("GDL_TUNING") == "1" and os.environ.get(name) == off)


def _partial_rows(eng, fn, M, ld):
    rows = getattr(eng.lib, fn)(eng.dt, M, ld)
    if rows <= 0:
        raise L.GdlError(f"{fn}: bad arguments (M = {M}, ld = {ld})")
    return rows


class _Linear:
    """One nn.Linear (weight [n][k], optional bias) over M rows, in the kernels' padded layouts.
    cs: when the bias gradient is a gdl_swin_colsum pass of this Linear's own -- "always"; "drop" (only in a backward with
    DropPath: otherwise it is the third result row of a LayerNorm backward); "pair" (always, unless the fused kernel of
    bwd_pair carries it); None (never)."""

    def __init__(self, eng, w_idx, b_idx, n, k, M, nseg=None, cs=None):
        self.eng, self.w_idx, self.b_idx, self.n, self.k, self.M = eng, w_idx, b_idx, n, k, M
        self.nseg, self.kseg = nseg or n, k
        self.nseg_pad, self.kseg_pad = _ld(self.nseg), _ld(self.kseg)
        self.np, self.kp = n // self.nseg * self.nseg_pad, k // self.kseg * self.kseg_pad
        dev, td = eng.device, eng.tdtype
        self.w = torch.empty((self.np, self.kp), dtype=td, device=dev)   # [out][in]  (forward, weight gradient)
        self.wT = torch.empty((self.kp, self.np), dtype=td, device=dev)  # [in][out]  (data gradient)
        self.b = torch.zeros(self.np, dtype=torch.float32, device=dev) if b_idx is not None else None
        self.dw = torch.empty((self.np, self.kp), dtype=torch.float32, device=dev)
        self.db = torch.empty(self.np, dtype=torch.float32, device=dev) if b_idx is not None else None
        # bwd_pair: both gradients from one pass over dy (csrc/linear_bwd.hip) where the shape is one of its; the bias gradient
        # rides in that kernel where the input width leaves it a padding tile
        self.fused = bool(eng.lib.gdl_linear_bwd_ok(eng.dt, M, self.kp, self.np))
        self.db_fused = cs == "pair" and self.fused and k <= 96
        self.cs = None if self.db_fused else "always" if cs == "pair" else cs
        self.cs_partial = None  # deferred folds: the column-sum pass leaves its partial rows here (SwinEngine._fold_all)
        if self.cs and eng.defer_folds:
            self.cs_rows = _partial_rows(eng, "gdl_swin_colsum_rows", M, self.np)
            self.cs_partial = torch.empty(self.cs_rows * self.np, dtype=torch.float32, device=dev)

    def pack_descs(self, params):
        """(src, dst, dstT, n, k, nseg, nseg_pad, kseg, kseg_pad, dtype) records of gdl_swin_pack_batched"""
        e = self.eng
        d = [(params[self.w_idx], self.w, self.wT, self.n, self.k, self.nseg, self.nseg_pad, self.kseg, self.kseg_pad, e.dt)]
        if self.b is not None:
            d.append((params[self.b_idx], self.b, None, self.n, 1, self.nseg, self.nseg_pad, 1, 1, L.GDL_F32))
        return d

    def unpack_descs(self, grads):
        d = [(self.dw, grads[self.w_idx], None, self.n, self.k, self.nseg, self.nseg_pad, self.kseg, self.kseg_pad, L.GDL_F32)]
        if self.b is not None:
            d.append((self.db, grads[self.b_idx], None, self.n, 1, self.nseg, self.nseg_pad, 1, 1, L.GDL_F32))
        return d

    def own_colsum(self, drop):
        """does a backward with / without DropPath run gdl_swin_colsum for this Linear's bias gradient?"""
        return self.cs == "always" or (self.cs == "drop" and drop)

    def fold_jobs(self, drop):
        """(partial, out, rows, width, stride) of gdl_swin_partial_reduce_batched"""
        return [(self.cs_partial, self.db, self.cs_rows, self.np, self.np)] if self.own_colsum(drop) else []

    def _table(self, mode):
        return L.ptr(self.eng.table(mode, self.M, self.kp, self.np))

    # y[M][np] = x[M][kp] . w^T
    def fwd(self, x, y, st):
        L.call("gdl_conv_fwd", self.eng.dt, L.ptr(x), L.ptr(self.w), L.ptr(y), None, self._table(L.GATHER_FWD), self.M, 1,
               1, self.kp, self.np, 1, 1, 1, 0, st)

    # y = x . w^T + b (+ res): bias and residual in the GEMM's epilogue
    def fwd_bias(self, x, y, res, st, gelu_out=None):
        L.call("gdl_conv_fwd_bias", self.eng.dt, L.ptr(x), L.ptr(self.w), L.ptr(y), L.ptr(self.b), L.ptr(res), L.ptr(gelu_out),
               self._table(L.GATHER_FWD), self.M, 1, 1, self.kp, self.np, 1, 1, 1, 0, st)

    # dx[M][kp] = dy[M][np] . w
    def dgrad(self, dy, dx, st):
        L.call("gdl_conv_dgrad", self.eng.dt, L.ptr(dy), L.ptr(self.wT), L.ptr(dx), None, self._table(L.GATHER_DGRAD),
               self.M, 1, 1, self.kp, self.np, 1, 1, 1, 0, st)

    # dx[M][kp] = (dy[M][np] . w) * gelu'(u), column sums of dx added to the fixed-point accumulators `acc` ([kp][2] int64)
    def dgrad_gelu(self, dy, dx, u, acc, scale, st):
        L.call("gdl_conv_dgrad_gelu", self.eng.dt, L.ptr(dy), L.ptr(self.wT), L.ptr(dx), L.ptr(u), L.ptr(acc), scale,
               self._table(L.GATHER_DGRAD), self.M, 1, 1, self.kp, self.np, 1, 1, 1, 0, st)

    # dx = dy . w, dw = dy^T . x; colsum (= own_colsum(drop) of a "pair" Linear): db = column sums of dy as well
    def bwd_pair(self, dy, x, dx, st, colsum=False):
        e = self.eng
        if self.fused:
            L.call("gdl_linear_bwd", e.dt, L.ptr(dy), L.ptr(x), L.ptr(self.wT), L.ptr(dx), L.ptr(self.dw),
                   L.ptr(self.db) if self.db_fused else None, L.ptr(e._lbws), e._lbws.numel(), self.M, self.kp, self.k, self.np, st)
            if colsum:
                self.colsum(dy, None, st)
        else:
            if colsum:
                self.colsum(dy, None, st)
            self.wgrad(dy, x, st)
            self.dgrad(dy, dx, st)

    # dw[np][kp] = dy^T . x
    def wgrad(self, dy, x, st):
        e = self.eng
        L.call("gdl_conv_wgrad", e.dt, L.ptr(dy), L.ptr(x), L.ptr(self.dw), self._table(L.GATHER_FWD), self.M, 1, 1,
               self.kp, self.np, 1, 1, 1, 0, L.ptr(e._wg), e._wg.numel(), st)

    def colsum(self, g, u, st):
        """db = column sums of g [M][np] (u given: g <- g * gelu'(u) first)"""
        e = self.eng
        if not e.defer_folds:
            L.call("gdl_swin_colsum", e.dt, L.ptr(g), L.ptr(u), L.ptr(self.db), L.ptr(e.partial), self.M, self.np, st)
            return
        if self.cs_partial is None:
            raise L.GdlError("SwinEngine: a column-sum pass that the fold plan does not have")
        L.call("gdl_swin_colsum", e.dt, L.ptr(g), L.ptr(u), None, L.ptr(self.cs_partial), self.M, self.np, st)


class _Norm:
    """One nn.LayerNorm over M rows.  colsum: its backward also returns the column sums of dx (dgb[2]) -- the bias gradient
    of `cs_lin`, the Linear whose output gradient dx is."""

    def __init__(self, eng, w_idx, b_idx, c, M, colsum):
        self.eng, self.w_idx, self.b_idx, self.c, self.ld, self.M, self.colsum = eng, w_idx, b_idx, c, _ld(c), M, colsum
        self.cs_lin = None
        dev = eng.device
        self.g = torch.zeros(self.ld, dtype=torch.float32, device=dev)
        self.b = torch.zeros(self.ld, dtype=torch.float32, device=dev)
        self.dgb = torch.empty((3, self.ld), dtype=torch.float32, device=dev)  # d gamma, d beta, (colsum) column sums of dx
        if eng.defer_folds:  # the partial rows stay in a buffer of this LayerNorm's own; SwinEngine._fold_all folds them
            self.rows = _partial_rows(eng, "gdl_swin_ln_bwd_rows", M, self.ld)
            self.partial = torch.empty(self.rows * 3 * self.ld, dtype=torch.float32, device=dev)

    def pack_descs(self, params):
        return [(params[src], dst, None, self.c, 1, self.c, self.ld, 1, 1, L.GDL_F32) for src, dst in ((self.w_idx, self.g), (self.b_idx, self.b))]

    def unpack_descs(self, grads):
        return [(self.dgb[row], grads[dst], None, self.c, 1, self.c, self.ld, 1, 1, L.GDL_F32) for row, dst in ((0, self.w_idx), (1, self.b_idx))]

    def fold_jobs(self, drop):
        """DropPath: the column sums of the scaled branch gradient (cs_lin's own pass) replace the third row, which sums the
        unscaled dx -- the kernel still leaves it at pitch 3 * ld, the fold stops in front of it"""
        nr = 3 if self.colsum else 2
        taken = self.colsum and self.cs_lin.own_colsum(drop)
        return [(self.partial, self.dgb, self.rows, (2 if taken else nr) * self.ld, nr * self.ld)]

    def fwd(self, x, y, stats, st):
        L.call("gdl_swin_ln_fwd", self.eng.dt, L.ptr(x), L.ptr(self.g), L.ptr(self.b), L.ptr(y), L.ptr(stats), self.M, self.c, self.ld, st)

    def bwd(self, dy, x, stats, add, dx, st):
        e = self.eng
        out, partial = (None, self.partial) if e.defer_folds else (self.dgb, e.partial)
        L.call("gdl_swin_ln_bwd_colsum" if self.colsum else "gdl_swin_ln_bwd", e.dt, L.ptr(dy), L.ptr(x), L.ptr(stats), L.ptr(self.g),
               L.ptr(add), L.ptr(dx), L.ptr(out), L.ptr(partial), self.M, self.c, self.ld, st)


class _Block:
    """One Swin block: its layers and what its forward saves for the backward."""
    __slots__ = ("k", "shift", "x_in", "norm1", "table_idx", "qkv", "proj", "norm2", "fc1", "fc2", "stats1", "h", "qkv_a", "attn",
                 "x_mid", "stats2", "m", "u", "a", "x_out", "fc1_off")

    def __init__(self, eng, pre, k, shift, x_in, C, hid, nh, nrel, M, norm1_cs, fc2_cs):
        """k: index among all blocks (row of drop_buf); x_in: the previous block's output; fc2_cs: see _Linear"""
        reg, buf, ld = eng._reg, eng._buf, _ld(C)
        self.k, self.shift, self.x_in = k, shift, x_in
        self.norm1 = _Norm(eng, reg(pre + "norm1.weight", (C,)), reg(pre + "norm1.bias", (C,)), C, M, norm1_cs)
        self.table_idx = reg(pre + "attn.relative_position_bias_table", (nrel, nh))
        self.qkv = _Linear(eng, reg(pre + "attn.qkv.weight", (3 * C, C)), reg(pre + "attn.qkv.bias", (3 * C,)), 3 * C, C, M, nseg=C, cs="pair")
        self.proj = _Linear(eng, reg(pre + "attn.proj.weight", (C, C)), reg(pre + "attn.proj.bias", (C,)), C, C, M,
                            cs="drop" if eng.fuse_ln else "always")
        self.norm2 = _Norm(eng, reg(pre + "norm2.weight", (C,)), reg(pre + "norm2.bias", (C,)), C, M, eng.fuse_ln)
        self.fc1 = _Linear(eng, reg(pre + "mlp.fc1.weight", (hid, C)), reg(pre + "mlp.fc1.bias", (hid,)), hid, C, M,
                           cs=None if eng.fuse_gelu else "always")
        self.fc2 = _Linear(eng, reg(pre + "mlp.fc2.weight", (C, hid)), reg(pre + "mlp.fc2.bias", (C,)), C, hid, M, cs=fc2_cs)
        self.stats1, self.h, self.qkv_a, self.attn = buf(M, 2, torch.float32), buf(M, ld), buf(M, 3 * ld), buf(M, ld)
        self.x_mid, self.stats2, self.m = buf(M, ld), buf(M, 2, torch.float32), buf(M, ld)
        self.u, self.a, self.x_out = buf(M, _ld(hid)), buf(M, _ld(hid)), buf(M, ld)


class _Stage:
    """The blocks at one resolution and, below the last stage, the patch merging behind them (red is None in the last)."""
    __slots__ = ("C", "r", "ws", "nh", "M", "ld", "hid", "blocks", "red", "mnorm", "cat", "catn", "mstats", "merged")

    def __init__(self, C, r, ws, nh, M, hid):
        self.C, self.r, self.ws, self.nh, self.M, self.ld, self.hid = C, r, ws, nh, M, _ld(C), hid
        self.blocks, self.red = [], None


class SwinEngine:
    """A planned Swin encoder for fixed (cfg, dtype, B, T).  `cfg`: dict(img, patch, embed, depths, heads, window, mlp).
    Parameters / gradients are lists of float32 CUDA tensors in the reference's named_parameters() order
    (`param_shapes()`); forward(x [B,3,T,img,img] f32) -> float32 [B*T, C_last]; backward(dfeat, grads)."""

    def __init__(self, cfg, dtype, B, T, device):
        self.lib = L.load()
        E, p, nl = cfg["embed"], cfg["patch"], len(cfg["depths"])
        if cfg["img"] % p != 0 or 3 * p * p > 64:
            raise L.GdlError(f"SwinEngine: img {cfg['img']} must be a multiple of patch {p}, and 3 * patch^2 at most 64")
        if any(E << i != nh * 32 for i, nh in enumerate(cfg["heads"])):
            raise L.GdlError(f"SwinEngine: head dimension must be 32 (embed {E}, heads {list(cfg['heads'])})")
        self.cfg, self.B, self.T = dict(cfg), B, T
        self.N = N = B * T
        self.dt = L.dtype_code(dtype)
        self.tdtype = L.torch_dtype(self.dt)
        self.device = dev = torch.device(device)
        # HIP-graph replay of the forward / backward launch sequences (see _run); GDL_NOGRAPH=1 (with GDL_TUNING=1) keeps every
        # pass eager -- the PMC scripts set it, so that counters are collected over ordinary launches
        self._graphs = {}
        self.use_graph = _knob("GDL_NOGRAPH", "1")
        # Round 6: the folds of the LayerNorm backwards' and column-sum passes' partial rows (42 launches per Swin-T backward, each
        # on the branch's only chain, each producing a parameter gradient nobody reads before the optimizer) wait until the end of
        # the backward and run as ONE launch (gdl_swin_partial_reduce_batched; a partial buffer per call site instead of the shared
        # one; bit-identical results).  GDL_SWIN_DEFER_FOLDS=0 (tuning aid): a fold launch behind every pass, as before.
        self.defer_folds = _knob("GDL_SWIN_DEFER_FOLDS", "0")
        # fc1 bias gradients: fixed-point column-sum accumulators of the fused fc2 data gradient (gdl_conv_dgrad_gelu)
        # (tuning aid, OFF by default: measured 26.8 ms either way at 192 frames -- the Linears' three GEMMs are all HBM-bound, beside
        # the weight gradients the data gradients slow down by what the weight gradients would have taken: 4.2 -> 6.4 ms)
        self.fuse_gelu = _knob("GDL_SWIN_FUSE_GELU", "0")
        # Bias gradients of the Linears fed by the residual stream's gradient (fc2, proj, the patch embedding) = a third result
        # row of the LayerNorm backward that produced that gradient
        self.fuse_ln = ln = _knob("GDL_SWIN_FUSE_LN", "0")
        self.serial = 0  # forward counter: a backward must follow the forward whose activations are in the buffers
        self.names = []
        buf, reg = self._buf, self._reg
        # ---- patch embedding
        res = cfg["img"] // p
        M0 = N * res * res
        self.pe = _Linear(self, reg("patch_embed.proj.weight", (E, 3, p, p)), reg("patch_embed.proj.bias", (E,)), E, 3 * p * p, M0,
                          cs=None if ln else "always")
        self.pe_norm = _Norm(self, reg("patch_embed.norm.weight", (E,)), reg("patch_embed.norm.bias", (E,)), E, M0, ln)
        self.pe_rows = buf(M0, 64)
        self.pe_out = buf(M0, _ld(E))
        self.pe_stats = buf(M0, 2, torch.float32)
        self.x0 = buf(M0, _ld(E))
        # ---- stages
        self.stages = []
        maxw, maxld = 0, 64
        xcur = self.x0
        for i, (depth, nh) in enumerate(zip(cfg["depths"], cfg["heads"])):
            C, r = E << i, res >> i
            s = _Stage(C, r, min(cfg["window"], r), nh, N * r * r, cfg["mlp"] * C)
            for j in range(depth):
                # this block's fc2 gets its bias gradient from the norm1 backward of the NEXT block (or the final norm's) -- not at a
                # stage's last block below the last stage (patch merging in between)
                rides = ln and (j + 1 < depth or i == nl - 1)
                s.blocks.append(_Block(self, f"layers.{i}.blocks.{j}.", sum(cfg["depths"][:i]) + j,
                                       0 if (j % 2 == 0 or r <= cfg["window"]) else cfg["window"] // 2, xcur, C, s.hid, nh,
                                       (2 * s.ws - 1) ** 2, s.M, ln and j > 0, "drop" if rides else "always"))
                xcur = s.blocks[-1].x_out
            maxld = max(maxld, 3 * s.ld, _ld(s.hid))
            if i < nl - 1:
                pre, M4 = f"layers.{i}.downsample.", s.M // 4
                s.red = _Linear(self, reg(pre + "reduction.weight", (2 * C, 4 * C)), None, 2 * C, 4 * C, M4)
                s.mnorm = _Norm(self, reg(pre + "norm.weight", (4 * C,)), reg(pre + "norm.bias", (4 * C,)), 4 * C, M4, False)
                s.cat, s.catn, s.mstats = buf(M4, 4 * C), buf(M4, 4 * C), buf(M4, 2, torch.float32)
                xcur = s.merged = buf(M4, _ld(2 * C))
                maxld = max(maxld, 4 * C)
            self.stages.append(s)
            maxw = max(maxw, self.lib.gdl_swin_attn_bwd_workspace_bytes(N, r, r, s.ws, nh))
        Cl, last = E << (nl - 1), self.stages[-1]
        self.out_norm = _Norm(self, reg("norm.weight", (Cl,)), reg("norm.bias", (Cl,)), Cl, last.M, ln)
        self.x_last = xcur
        self.out_stats, self.out_ln = buf(last.M, 2, torch.float32), buf(last.M, last.ld)
        self.feat = torch.empty((N, Cl), dtype=torch.float32, device=dev)
        self.feat_b = torch.empty((B, Cl), dtype=torch.float32, device=dev)  # averaged over the T frames of a sample
        self.C_out, self.L_out = Cl, last.r * last.r
        # scratch: LayerNorm / column-sum partials (per-call folds), attention table partials, gradient buffers
        self.partial = torch.empty(self.lib.gdl_swin_partial_bytes(maxld), dtype=torch.uint8, device=dev)
        self.tpart = torch.empty(max(maxw, 4), dtype=torch.uint8, device=dev)
        td, M1, ld1 = self.tdtype, self.stages[0].M, self.stages[0].ld
        wide = max(max(3 * s.ld, _ld(s.hid)) * s.M for s in self.stages)
        self.g_a = torch.empty(M1 * ld1, dtype=td, device=dev)   # gradient of the residual stream (ping)
        self.g_b = torch.empty(M1 * ld1, dtype=td, device=dev)   # (pong)
        self.g_c = torch.empty(M1 * ld1, dtype=td, device=dev)   # branch gradient at token width
        self.g_w = torch.empty(wide, dtype=td, device=dev)       # branch gradient at QKV / hidden width
        self.g_cat = torch.empty(max([s.M // 4 * 4 * s.C for s in self.stages[:-1]] + [1]), dtype=td, device=dev)
        self.g_cat2 = torch.empty_like(self.g_cat)
        # fuse_gelu: one accumulator arena for all blocks (zeroed / converted once per backward phase); the float results ARE the
        # Linears' db buffers (views)
        tot = 0
        self.fc1_off = []
        for s in self.stages:
            for b in s.blocks:
                b.fc1_off = tot
                tot += b.fc1.np
            self.fc1_off.append(tot)  # end offset of the stage
        self.fc1_acc = torch.zeros((tot, 2), dtype=torch.int64, device=dev)
        self.fc1_db = torch.zeros(tot, dtype=torch.float32, device=dev)
        # |mean over the rows| < 2^7 for every column of a hidden-width gradient; one scale for all stages (the widest M)
        self.fc1_scale = 2.0 ** (62 - 7 - max(1, (M1 - 1).bit_length()))
        if self.fuse_gelu:
            for s in self.stages:
                for b in s.blocks:
                    b.fc1.db = self.fc1_db[b.fc1_off:b.fc1_off + b.fc1.np]
        # fuse_ln: every LayerNorm whose backward has the column-sum form hands its third row to the Linear it feeds
        carried = [(self.pe_norm, self.pe)]
        for s in self.stages:
            after = [b.norm1 for b in s.blocks[1:]] + ([self.out_norm] if s is last else [])  # (none behind a patch merging)
            carried += [(b.norm2, b.proj) for b in s.blocks] + [(norm, b.fc2) for norm, b in zip(after, s.blocks)]
        for norm, lin in carried:
            if norm.colsum:
                lin.db, norm.cs_lin = norm.dgb[2], lin
        linears = [o for o in self._linears_norms() if isinstance(o, _Linear)]
        # the weight gradients' split-K workspace, the partials of the fused data + weight gradient (csrc/linear_bwd.hip) and the
        # 1x1 convolutions' gather tables, for every shape the passes launch
        self._wg = torch.empty(max(self.lib.gdl_conv_wgrad_workspace_bytes(self.dt, o.M, 1, 1, o.kp, o.np, 1, 1, 1, 0) for o in linears),
                               dtype=torch.uint8, device=dev)
        self._lbws = torch.empty(max([self.lib.gdl_linear_bwd_workspace_bytes(o.M, o.kp, o.np) for o in linears if o.fused] + [16]),
                                 dtype=torch.uint8, device=dev)
        self._tables = {}
        for o in linears:
            for mode in (L.GATHER_FWD, L.GATHER_DGRAD):
                key = self._table_key(mode, o.M, o.kp, o.np)
                if key not in self._tables:
                    t = torch.empty(self.lib.gdl_conv_table_bytes(mode, o.M, 1, 1, 1, 1, 1, 0), dtype=torch.uint8, device=dev)
                    L.call("gdl_conv_build_table", mode, self.dt, o.M, 1, 1, o.kp, o.np, 1, 1, 1, 0, L.ptr(t), L.cur_stream())
                    self._tables[key] = t
        # deferred folds: one table of jobs per backward body -- (part of _linears_norms, DropPath)
        self._fold_tabs = {}
        if self.defer_folds:
            for part in (None, "last", "rest"):
                for drop in (False, True):
                    self._fold_tabs[part, drop] = self._fold_table([j for o in self._linears_norms(part) for j in o.fold_jobs(drop)])
        torch.cuda.current_stream(dev).synchronize()  # (the tables are read on whichever stream a pass runs on)
        self._params = None
        self._pack_key, self._pack_tab, self._unpack_tabs = None, None, {}  # desc tables, cached by the caller's pointers
        self.have_fwd = False
        self._bw_phase1_serial = None
        # stochastic depth (swin_transformer.py:218, 290, 293): per-frame scales of the two residual branches of every block, copied
        # here from the caller's tensor by a forward that is given one (fixed address: the launch sequences may be graph replays)
        self.nblocks = sum(cfg["depths"])
        self.drop_buf = torch.ones((self.nblocks, 2, N), dtype=torch.float32, device=dev)
        self._drop = False  # the last forward ran with DropPath: its backward scales the branch gradients the same way

    # ------------------------------------------------------------------ plumbing
    def _reg(self, name, shape):
        self.names.append((name, tuple(shape)))
        return len(self.names) - 1

    def _buf(self, rows, cols, dtype=None):
        return torch.empty((rows, cols), dtype=dtype or self.tdtype, device=self.device)

    def param_shapes(self):
        return list(self.names)

    @staticmethod
    def _table_key(mode, M, C, K):
        return mode, M, C if mode == L.GATHER_FWD else K

    def table(self, mode, M, C, K):
        t = self._tables.get(self._table_key(mode, M, C, K))
        if t is None:
            raise L.GdlError(f"SwinEngine: no gather table (mode {mode}) for {M} rows, {C} -> {K} channels")
        return t

    def set_params(self, params):
        if len(params) != len(self.names):
            raise L.GdlError(f"SwinEngine.set_params: {len(params)} tensors, expected {len(self.names)}")
        for p, (n, shape) in zip(params, self.names):
            if p.dtype != torch.float32 or not p.is_contiguous() or tuple(p.shape) != shape or p.device != self.device:
                raise L.GdlError(f"SwinEngine.set_params: {n} must be a contiguous float32 tensor of shape {shape} on {self.device}")
        self._params = list(params)

    def _to_device(self, arr):
        return torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(self.device)

    def _desc_table(self, recs, unpack):
        """device array of SwinPackDesc + its block count (1024 elements per block)"""
        arr = (_PackDesc * len(recs))()
        blk = 0
        for d, (src, dst, dstT, n, k, nseg, nseg_pad, kseg, kseg_pad, dt) in zip(arr, recs):
            d.src, d.dst, d.dstT = src.data_ptr(), dst.data_ptr(), (dstT.data_ptr() if dstT is not None else None)
            d.n, d.k, d.nseg, d.nseg_pad, d.kseg, d.kseg_pad = n, k, nseg, nseg_pad, kseg, kseg_pad
            d.np, d.kp, d.dt, d.blk0 = n // nseg * nseg_pad, k // kseg * kseg_pad, dt, blk
            blk += ((n * k if unpack else d.np * d.kp) + 1023) // 1024
        return self._to_device(arr), len(recs), blk

    def _pack_all(self, st):
        key = tuple(p.data_ptr() for p in self._params)
        if self._pack_key != key:
            recs = [r for o in self._linears_norms() for r in o.pack_descs(self._params)]
            self._pack_tab, self._pack_key = self._desc_table(recs, False), key
        t, n, blk = self._pack_tab
        L.call("gdl_swin_pack_batched", L.ptr(t), n, blk, 0, st)

    def _unpack_all(self, grads, st, part=None):
        key = tuple(g.data_ptr() for g in grads)
        cache = self._unpack_tabs
        if cache.get("key") != key:
            cache.clear()
            cache["key"] = key
        if part not in cache:
            recs = [r for o in self._linears_norms(part) for r in o.unpack_descs(grads)]
            cache[part] = self._desc_table(recs, True)
        t, n, blk = cache[part]
        L.call("gdl_swin_pack_batched", L.ptr(t), n, blk, 1, st)

    # ------------------------------------------------------------------ deferred folds of partial rows
    def _fold_table(self, jobs):
        """device array of SwinRedDesc + its block count (16 columns per block); the jobs are independent: no result range may
        meet another's"""
        arr = (_RedDesc * len(jobs))()
        blk, spans = 0, []
        for d, (partial, out, rows, width, stride) in zip(arr, jobs):
            d.partial, d.out, d.rows, d.width, d.blk0, d.stride = partial.data_ptr(), out.data_ptr(), rows, width, blk, stride
            blk += (width + 15) // 16
            spans.append((d.out, d.out + 4 * width))
        spans.sort()
        if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
            raise L.GdlError("SwinEngine: overlapping fold results")
        return self._to_device(arr), len(jobs), blk

    def _fold_all(self, st, part, drop):
        """one launch: every deferred fold of this backward body (before its gradients are unpacked)"""
        if self.defer_folds:
            t, n, blk = self._fold_tabs[part, drop]
            L.call("gdl_swin_partial_reduce_batched", L.ptr(t), n, blk, st)

    def _linears_norms(self, part=None):
        """part None: every Linear / LayerNorm; "last": the last stage's blocks and the final norm (the parameters whose
        gradients backward phase 1 completes -- DGLTrainer's visual_l4 bucket); "rest": the others."""
        last = len(self.stages) - 1
        if part != "last":
            yield self.pe
            yield self.pe_norm
        for si, s in enumerate(self.stages):
            if part is None or (part == "last") == (si == last):
                for b in s.blocks:
                    yield from (b.norm1, b.qkv, b.proj, b.norm2, b.fc1, b.fc2)
            if s.red is not None and part != "last":
                yield s.red
                yield s.mnorm
        if part != "rest":
            yield self.out_norm

    def _v(self, flat, rows, cols):
        return flat[:rows * cols].view(rows, cols)

    # ------------------------------------------------------------------ forward
    def forward(self, x, pool_frames=False, out=None, drop_scales=None):
        """-> float32 [B*T, C_last] (the reference's contract), or [B, C_last] averaged over the frames of a sample
        (pool_frames: what basic_model.py:77-80 does for the ResNet branch -- the samples' frames are consecutive rows).
        drop_scales: None (DropPath is the identity: eval mode, or drop_path_rate = 0) or a float32 [blocks][2][B*T] tensor on
        the device -- the factor each frame's attention / Mlp branch is multiplied with before it joins the residual stream, 0
        or 1 / keep_prob (timm's drop_path with scale_by_keep; the caller draws them: `models.swin_transformer.drop_path_scales`)."""
        if self._params is None:
            raise L.GdlError("SwinEngine.forward: parameters not set")
        cfg, dt, N, st = self.cfg, self.dt, self.N, L.cur_stream()
        B, T = self.B, self.T
        if tuple(x.shape) != (B, 3, T, cfg["img"], cfg["img"]) or x.dtype != torch.float32 or not x.is_contiguous() or \
                x.device != self.device:
            raise L.GdlError("SwinEngine.forward: x must be a contiguous float32 [B, 3, T, img, img] tensor on the engine's device")
        if out is None:
            out = self.feat_b if pool_frames else self.feat
        elif tuple(out.shape) != ((B if pool_frames else N), self.C_out) or out.dtype != torch.float32 or not out.is_contiguous():
            raise L.GdlError("SwinEngine.forward: `out` must be a contiguous float32 [B*T or B, C_last] tensor")
        drop = drop_scales is not None
        if drop:
            if tuple(drop_scales.shape) != tuple(self.drop_buf.shape) or drop_scales.dtype != torch.float32 or \
                    drop_scales.device != self.device:
                raise L.GdlError(f"SwinEngine.forward: drop_scales must be a float32 {list(self.drop_buf.shape)} tensor on the engine's device")
            self.drop_buf.copy_(drop_scales, non_blocking=True)
        self._drop = drop
        L.call("gdl_swin_patch_gather", dt, L.ptr(x), L.ptr(self.pe_rows), B, T, cfg["img"], cfg["img"], cfg["patch"], st)
        key = ("f", out.data_ptr(), bool(pool_frames), drop) + tuple(p.data_ptr() for p in self._params)
        self._run(key, lambda: self._forward_body(out, pool_frames, drop))
        self.have_fwd = True
        self.serial += 1
        return out

    def _run(self, key, body):
        """Run `body` (a fixed launch sequence over fixed buffers) -- eagerly the first two times and whenever the
        measurement tap is recording, afterwards as a replay of its captured HIP graph: ~400 launches per pass enqueued from
        Python would otherwise leave the device waiting for the host."""
        if not self.use_graph or self.lib.gdl_prof_enabled():
            return body()
        ent = self._graphs.get(key)
        if ent is None:
            if len(self._graphs) >= 8:  # callers that pass fresh buffers every time (autograd) never repeat a key
                self._graphs = {k: v for k, v in self._graphs.items() if v["g"] is not None}
                if len(self._graphs) >= 8:
                    return body()
            ent = self._graphs[key] = {"n": 0, "g": None}
        if ent["g"] is not None:
            return ent["g"].replay()
        ent["n"] += 1
        if ent["n"] <= 2:
            return body()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g):
                body()
        except RuntimeError as e:  # capture not possible on this stack: stay eager from here on
            self.use_graph = False
            torch.cuda.synchronize(self.device)
            if torch.cuda.is_current_stream_capturing():
                raise L.GdlError(f"SwinEngine: graph capture failed and the stream is still capturing: {e}") from e
            return body()
        ent["g"] = g
        g.replay()

    def _drop_path(self, y, res, k, branch, out, M, ld, st):
        """out = (res or 0) + drop_buf[k][branch][frame of the row] * y"""
        L.call("gdl_swin_drop_path", self.dt, L.ptr(y), L.ptr(res) if res is not None else None, L.ptr(self.drop_buf[k, branch]),
               L.ptr(out), M, M // self.N, ld, st)

    def _forward_body(self, out, pool_frames, drop=False):
        dt, N, st = self.dt, self.N, L.cur_stream()
        B, T = self.B, self.T
        P = self._params
        self._pack_all(st)  # float32 masters -> kernel layouts (one launch per step, like the encoder's weight pack)
        self.pe.fwd_bias(self.pe_rows, self.pe_out, None, st)
        self.pe_norm.fwd(self.pe_out, self.x0, self.pe_stats, st)
        for s in self.stages:
            M, ld, r = s.M, s.ld, s.r
            for b in s.blocks:
                b.norm1.fwd(b.x_in, b.h, b.stats1, st)
                b.qkv.fwd_bias(b.h, b.qkv_a, None, st)
                L.call("gdl_swin_attn_fwd", dt, L.ptr(b.qkv_a), L.ptr(P[b.table_idx]), L.ptr(b.attn), N, r, r, s.ws, b.shift, s.nh, ld, st)
                if drop:  # the branch without the residual, then x_mid = x_in + scale[frame] * branch (g_c: free during a forward)
                    br = self._v(self.g_c, M, ld)
                    b.proj.fwd_bias(b.attn, br, None, st)
                    self._drop_path(br, b.x_in, b.k, 0, b.x_mid, M, ld, st)
                else:
                    b.proj.fwd_bias(b.attn, b.x_mid, b.x_in, st)
                b.norm2.fwd(b.x_mid, b.m, b.stats2, st)
                b.fc1.fwd_bias(b.m, b.u, None, st, gelu_out=b.a)  # u = fc1(m) + b, a = gelu(u)
                if drop:
                    b.fc2.fwd_bias(b.a, br, None, st)
                    self._drop_path(br, b.x_mid, b.k, 1, b.x_out, M, ld, st)
                else:
                    b.fc2.fwd_bias(b.a, b.x_out, b.x_mid, st)
            if s.red is not None:
                L.call("gdl_swin_merge", dt, L.ptr(s.blocks[-1].x_out), L.ptr(s.cat), N, r, r, s.C, ld, 0, st)
                s.mnorm.fwd(s.cat, s.catn, s.mstats, st)
                s.red.fwd(s.catn, s.merged, st)
        self.out_norm.fwd(self.x_last, self.out_ln, self.out_stats, st)
        L.call("gdl_swin_token_mean", dt, L.ptr(self.out_ln), L.ptr(out), B if pool_frames else N,
               self.L_out * (T if pool_frames else 1), self.C_out, self.stages[-1].ld, st)

    # ------------------------------------------------------------------ backward
    def backward(self, dfeat, grads, serial=None, phase=0):
        """dfeat float32 [B*T, C_last] (or [B, C_last] for a pool_frames forward); grads: float32 tensors of the
        parameter shapes (overwritten).  serial: the engine's `serial` right after the forward being differentiated -- if
        another forward has run through the engine since (a validation pass of the same shape, two forwards before one
        backward), its activations are gone and this raises instead of returning gradients of the wrong pass.
        phase 0: the whole backward.  phase 1: the upstream gradient, the final norm and the LAST stage -- afterwards the gradients
        of `layers.<last>.*` and `norm.*` (half of Swin-T's parameters) are final on the stream, so a data-parallel caller
        can start their all-reduce (DGLTrainer's visual_l4 bucket) while phase 2 (the other stages and the patch embedding;
        same `dfeat` / `grads` arguments) runs -- the counterpart of gdl_encoder_backward_phase."""
        if not self.have_fwd:
            raise L.GdlError("SwinEngine.backward: no forward to differentiate")
        if serial is not None and serial != self.serial:
            raise L.GdlError("SwinEngine.backward: the engine has run another forward since the one being differentiated "
                             f"(forward {serial}, now {self.serial}): its saved activations were overwritten")
        if len(grads) != len(self.names):
            raise L.GdlError("SwinEngine.backward: wrong number of gradient tensors")
        N = self.N
        pooled = dfeat.shape[0] == self.B and self.T > 1
        if tuple(dfeat.shape) != ((self.B if pooled else N), self.C_out) or dfeat.dtype != torch.float32 or not dfeat.is_contiguous():
            raise L.GdlError("SwinEngine.backward: dfeat must be a contiguous float32 [B*T or B, C_last] tensor")
        for gten, (n, shape) in zip(grads, self.names):
            if gten.dtype != torch.float32 or not gten.is_contiguous() or tuple(gten.shape) != shape:
                raise L.GdlError(f"SwinEngine.backward: the gradient of {n} must be a contiguous float32 tensor of shape {shape}")
        if phase not in (0, 1, 2):
            raise L.GdlError("SwinEngine.backward: phase must be 0, 1 or 2")
        if phase == 2 and self._bw_phase1_serial != self.serial:
            raise L.GdlError("SwinEngine.backward: phase 2 without phase 1 of the same forward")
        if phase == 1:
            self._bw_phase1_serial = self.serial
        grads = list(grads)
        key = ("b", phase, dfeat.data_ptr(), pooled, self._drop) + tuple(t.data_ptr() for t in grads) + tuple(p.data_ptr() for p in self._params)
        self._run(key, lambda: self._backward_body(dfeat, grads, pooled, phase, self._drop))
        if phase == 2:
            self._bw_phase1_serial = None

    def _backward_body(self, dfeat, grads, pooled, phase=0, drop=False):
        dt, N, st = self.dt, self.N, L.cur_stream()
        P = self._params
        last = self.stages[-1]
        nst = len(self.stages)
        M, ld = last.M, last.ld
        ga, gb = self._v(self.g_a, M, ld), self._v(self.g_b, M, ld)
        if phase != 2:
            L.call("gdl_swin_token_mean_bwd", dt, L.ptr(dfeat), L.ptr(ga), self.B if pooled else N,
                   self.L_out * (self.T if pooled else 1), self.C_out, ld, st)
            self.out_norm.bwd(ga, self.x_last, self.out_stats, None, gb, st)
        # dx: gradient of the current stage's output tokens.  (Every block hands dx back in the buffer it got it in, so after
        # the last stage it sits in g_b again: phase 2 picks it up there without any state from phase 1 -- both phases may
        # be HIP-graph replays.)
        dx, spare = gb, ga
        first_si = nst - 2 if phase == 2 else nst - 1
        last_si = nst - 1 if phase == 1 else 0
        fuse = self.fuse_gelu
        acc_lo = self.fc1_off[last_si - 1] if last_si > 0 else 0
        acc_hi = self.fc1_off[first_si]
        if fuse:
            self.fc1_acc[acc_lo:acc_hi].zero_()
        for si in range(first_si, last_si - 1, -1):
            s = self.stages[si]
            M, ld, r = s.M, s.ld, s.r
            if s.red is not None:  # dx is the gradient of the merged tokens [M/4][ld(2C)]
                M4, C4 = M // 4, 4 * s.C
                gc, gc2 = self._v(self.g_cat, M4, C4), self._v(self.g_cat2, M4, C4)
                s.red.wgrad(dx, s.catn, st)
                s.red.dgrad(dx, gc, st)
                s.mnorm.bwd(gc, s.cat, s.mstats, None, gc2, st)
                dx = self._v(self.g_a, M, ld)
                spare = self._v(self.g_b, M, ld)
                L.call("gdl_swin_merge", dt, L.ptr(gc2), L.ptr(dx), N, r, r, s.C, ld, 1, st)
            else:
                dx, spare = self._v(dx.reshape(-1), M, ld), self._v(spare.reshape(-1), M, ld)
            gtok = self._v(self.g_c, M, ld)
            for b in reversed(s.blocks):
                gw = self._v(self.g_w, M, b.fc1.np)
                # x_out = x_mid + fc2(gelu(fc1(norm2(x_mid)))) ; dx = d x_out
                # DropPath: the Mlp branch sees g2 = scale[frame] * dx (in gtok until d m is written there); its bias gradient is a
                # column sum of g2 -- the row the LayerNorm backward left for it sums the unscaled dx
                g2 = dx
                if drop:
                    g2 = gtok
                    self._drop_path(dx, None, b.k, 1, g2, M, ld, st)
                if b.fc2.own_colsum(drop):
                    b.fc2.colsum(g2, None, st)
                b.fc2.wgrad(g2, b.a, st)
                if fuse:  # d u = (dx . W2) * gelu'(u) and fc1's bias gradient in the GEMM's epilogue
                    b.fc2.dgrad_gelu(g2, gw, b.u, self.fc1_acc[b.fc1_off:], self.fc1_scale, st)
                else:
                    b.fc2.dgrad(g2, gw, st)        # d a
                if b.fc1.own_colsum(drop):
                    b.fc1.colsum(gw, b.u, st)      # d u
                b.fc1.bwd_pair(gw, b.m, gtok, st)  # fc1's weight gradient and d m
                b.norm2.bwd(gtok, b.x_mid, b.stats2, dx, spare, st)   # spare = d x_mid
                # x_mid = x_in + proj(attn(qkv(norm1(x_in))))
                g1 = spare
                if drop:  # g1 = scale[frame] * d x_mid, in g_w (free between fc1's data gradient and the attention backward)
                    g1 = self._v(self.g_w, M, ld)
                    self._drop_path(spare, None, b.k, 0, g1, M, ld, st)
                if b.proj.own_colsum(drop):
                    b.proj.colsum(g1, None, st)
                b.proj.wgrad(g1, b.attn, st)
                b.proj.dgrad(g1, gtok, st)         # d attention output
                gq = self._v(self.g_w, M, 3 * ld)
                L.call("gdl_swin_attn_bwd", dt, L.ptr(b.qkv_a), L.ptr(P[b.table_idx]), L.ptr(gtok), L.ptr(gq),
                       L.ptr(grads[b.table_idx]), L.ptr(self.tpart), N, r, r, s.ws, b.shift, s.nh, ld, st)
                b.qkv.bwd_pair(gq, b.h, gtok, st, colsum=b.qkv.own_colsum(drop))  # qkv's weight and bias gradients and d h
                b.norm1.bwd(gtok, b.x_in, b.stats1, spare, dx, st)    # dx = d x_in
        if fuse:
            L.call("gdl_acc_to_float", L.ptr(self.fc1_acc[acc_lo:]), acc_hi - acc_lo, 1.0 / self.fc1_scale, L.ptr(self.fc1_db[acc_lo:]), st)
        if phase == 1:
            self._fold_all(st, "last", drop)
            self._unpack_all(grads, st, "last")  # the last stage's and the final norm's gradients -> the parameters' shapes
            return
        # patch embedding: x0 = norm(conv(x) + b); no input gradient
        g0 = self._v(spare.reshape(-1), self.pe.M, self.pe.np)
        self.pe_norm.bwd(dx, self.pe_out, self.pe_stats, None, g0, st)
        if self.pe.own_colsum(drop):
            self.pe.colsum(g0, None, st)
        self.pe.wgrad(g0, self.pe_rows, st)
        part = "rest" if phase == 2 else None
        self._fold_all(st, part, drop)
        self._unpack_all(grads, st, part)  # padded float32 gradients -> the parameters' shapes, one launch
