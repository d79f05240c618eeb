"""The case list of the element-wise convolution tests -- ONE place, imported by tests/test_conv_ref_cpu.py (which proves on
the CPU that an fp32-accumulated result passes the bound for every case) and by tests/test_conv_elementwise_gpu.py (which
runs the kernels).  CPU only.

A case names the entry point, the storage type, the geometry, the options, the kernel slot the launch must reach (the names the
launchers of csrc/conv_igemm.hip register with the timing tap) and r, the roundings to the storage type on that path as read from
its epilogue code (conv_ref's docstring).  Shapes are the smallest that reach the kernel, its ragged last tile and its image
borders under plan_conv: when the planner changes and a case lands on another kernel, move the SHAPE, not the expectation."""
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_ref as cr

Case = namedtuple("Case", "id op dt shape slot r opt")

C64 = "gdl::conv3x3_c64_kernel<%s>"
PS = "gdl::conv3x3_pslab_kernel<%d, %d, %d, %d>"        # rows of the M-tile, MODE, slab buffers, RICH
SLAB = "gdl::conv3x3_slab_kernel<%s, %d, %d, %d, %d>"   # T, BM, BN, MODE, waves
FLAT = "gdl::conv_igemm_kernel<%s, %d, %d, %d, %d, %d>"  # T, BM, BN, WM, WN, MODE
STEM_PERS = "gdl::conv_stem_pers_kernel"
BF, FP = "gdl::bf16", "float"
_WAVES = {(64, 64): (2, 2), (128, 64): (2, 2), (256, 64): (4, 1), (128, 128): (2, 2)}


def flat(t, bm, bn, mode):
    return FLAT % ((t, bm, bn) + _WAVES[(bm, bn)] + (mode,))


def _c(id, op, dt, shape, slot, r=1, **opt):
    return Case(id, op, dt, shape, slot, r, opt)


# shape: N, C, H, W, K, R, stride, pad (the forward's geometry, also for data gradients); the stem: B, Cin, T, H, W
L1_ODD = (3, 64, 65, 47, 64, 3, 1, 1)       # M = 9165: 72 tiles of 128 on 512 blocks, ragged last tile, two slab buffers
L1_WIDE = (2, 64, 33, 157, 64, 3, 1, 1)     # 157 pixels wide: ONE slab buffer
ODD256 = (7, 256, 13, 11, 256, 3, 1, 1)     # M = 1001, two N-tiles, four channel chunks
S2_EVEN = (3, 64, 20, 18, 128, 3, 2, 1)
S2_ODD = (2, 64, 65, 47, 128, 3, 2, 1)

CASES = [
    # ---- conv3x3_c64_kernel
    _c("c64_fwd_ragged", "fwd", "bf16", L1_ODD, C64 % "0"),
    _c("c64_dgrad_ragged", "dgrad", "bf16", L1_ODD, C64 % "1"),
    _c("c64_fwd_one_slab", "fwd", "bf16", L1_WIDE, C64 % "0"),
    _c("c64_dgrad_one_slab", "dgrad", "bf16", L1_WIDE, C64 % "1"),
    _c("c64_dgrad_bn", "dgrad_bn", "bf16", L1_ODD, C64 % "1, true", bits=True),           # fp32 staging: r = 1
    _c("c64_dgrad_bn_one_slab", "dgrad_bn", "bf16", L1_WIDE, C64 % "1, true"),
    _c("c64_dgrad_addend", "dgrad", "bf16", L1_ODD, C64 % "1", r=2, addend=True),         # in place; bf16 staging + addend: r = 2
    _c("c64_dgrad_relu", "dgrad_relu", "bf16", L1_ODD, C64 % "1", r=2),
    # ---- conv3x3_pslab_kernel: 192-row tiles need M >= 127 * 192 + 1 rows at 128 output channels
    _c("ps192_fwd_ic64", "fwd", "bf16", (26, 64, 31, 31, 128, 3, 1, 1), PS % (192, 0, 1, 0)),
    _c("ps192_dgrad_ic64", "dgrad", "bf16", (26, 128, 31, 31, 64, 3, 1, 1), PS % (192, 1, 1, 0)),
    _c("ps192_fwd_ic128", "fwd", "bf16", (26, 128, 31, 31, 128, 3, 1, 1), PS % (192, 0, 1, 0)),   # the slab is reloaded per chunk
    _c("ps192_dgrad_ic128", "dgrad", "bf16", (26, 128, 31, 31, 128, 3, 1, 1), PS % (192, 1, 1, 0)),
    _c("ps192_dgrad_addend", "dgrad", "bf16", (26, 128, 31, 31, 64, 3, 1, 1), PS % (192, 1, 1, 1), r=2, addend=True),
    # 128-row tiles through the 8-wave plan
    _c("ps128_fwd_odd", "fwd", "bf16", ODD256, PS % (128, 0, 2, 0)),
    _c("ps128_dgrad_odd", "dgrad", "bf16", ODD256, PS % (128, 1, 2, 0)),
    _c("ps128_fwd_w24", "fwd", "bf16", (5, 128, 33, 24, 128, 3, 1, 1), PS % (128, 0, 2, 0)),     # M = 3960: 31 tiles, ragged
    _c("ps128_dgrad_w24", "dgrad", "bf16", (5, 128, 33, 24, 128, 3, 1, 1), PS % (128, 1, 2, 0)),
    _c("ps128_fwd_two_ntiles", "fwd", "bf16", (6, 256, 14, 14, 256, 3, 1, 1), PS % (128, 0, 2, 0)),
    _c("ps128_dgrad_two_ntiles", "dgrad", "bf16", (6, 256, 14, 14, 256, 3, 1, 1), PS % (128, 1, 2, 0)),
    _c("ps128_fwd_three_ntiles", "fwd", "bf16", (3, 128, 14, 14, 384, 3, 1, 1), PS % (128, 0, 2, 0)),   # 15 items on 16 blocks
    _c("ps128_dgrad_three_ntiles", "dgrad", "bf16", (3, 384, 14, 14, 128, 3, 1, 1), PS % (128, 1, 2, 0)),
    _c("ps128_fwd_one_slab", "fwd", "bf16", (2, 64, 17, 13, 128, 3, 1, 1), PS % (128, 0, 1, 0)),
    _c("ps128_dgrad_one_slab", "dgrad", "bf16", (2, 128, 17, 13, 64, 3, 1, 1), PS % (128, 1, 1, 0)),
    _c("ps128_dgrad_one_slab_addend", "dgrad", "bf16", (2, 128, 17, 13, 64, 3, 1, 1), PS % (128, 1, 1, 1), r=2, addend=True),
    _c("ps128_dgrad_rich_addend", "dgrad", "bf16", ODD256, PS % (128, 1, 2, 1), r=2, addend=True),
    _c("ps128_dgrad_rich_two_partners", "dgrad_bn", "bf16", ODD256, PS % (128, 1, 2, 1), bits=True, two=True),
    _c("ps128_dgrad_bn", "dgrad_bn", "bf16", (5, 128, 33, 24, 128, 3, 1, 1), PS % (128, 1, 2, 0), bits=True),
    # more items than blocks (775 on 512): a block walks two tiles
    _c("ps128_fwd_several_tiles", "fwd", "bf16", (91, 64, 33, 33, 128, 3, 1, 1), PS % (128, 0, 1, 0)),
    _c("ps128_dgrad_several_tiles", "dgrad", "bf16", (91, 128, 33, 33, 64, 3, 1, 1), PS % (128, 1, 1, 0)),
    # ---- conv3x3_slab_kernel, bf16, where the planner still chooses it
    _c("slab_bf16_128x64_fwd", "fwd", "bf16", (2, 128, 17, 13, 64, 3, 1, 1), SLAB % (BF, 128, 64, 0, 4)),
    _c("slab_bf16_128x64_dgrad", "dgrad", "bf16", (2, 64, 17, 13, 128, 3, 1, 1), SLAB % (BF, 128, 64, 1, 4)),
    _c("slab_bf16_128x64_dgrad_relu", "dgrad_relu", "bf16", (2, 64, 17, 13, 64, 3, 1, 1), SLAB % (BF, 128, 64, 1, 4), r=2),
    _c("slab_bf16_128x64_dgrad_bn", "dgrad_bn", "bf16", (2, 64, 17, 13, 64, 3, 1, 1), SLAB % (BF, 128, 64, 1, 4), bits=True),
    # an epilogue option moves a persistent plan to the slab kernel (y only; the GELU output keeps its own test)
    _c("slab_bf16_8w_fwd_bias", "fwd_bias", "bf16", (4, 128, 17, 12, 128, 3, 1, 1), SLAB % (BF, 128, 128, 0, 8), r=2),
    _c("slab_bf16_128x128_fwd_bias", "fwd_bias", "bf16", (94, 64, 31, 17, 128, 3, 1, 1), SLAB % (BF, 128, 128, 0, 4), r=2),
    _c("slab_bf16_128x64_fwd_bias", "fwd_bias", "bf16", L1_ODD, SLAB % (BF, 128, 64, 0, 4), r=2),
    # widths whose slab exceeds the persistent kernel's 32 KiB
    _c("slab_bf16_8w_fwd_wide", "fwd", "bf16", (2, 64, 9, 65, 128, 3, 1, 1), SLAB % (BF, 128, 128, 0, 8)),
    _c("slab_bf16_8w_dgrad_wide", "dgrad", "bf16", (2, 128, 9, 65, 64, 3, 1, 1), SLAB % (BF, 128, 128, 1, 8)),
    _c("slab_bf16_192_fwd_wide", "fwd", "bf16", (23, 64, 33, 33, 128, 3, 1, 1), SLAB % (BF, 192, 128, 0, 4)),
    _c("slab_bf16_192_dgrad_wide", "dgrad", "bf16", (23, 128, 33, 33, 64, 3, 1, 1), SLAB % (BF, 192, 128, 1, 4)),
    _c("slab_bf16_128x128_fwd_wide", "fwd", "bf16", (6, 64, 128, 65, 128, 3, 1, 1), SLAB % (BF, 128, 128, 0, 4)),
    _c("slab_bf16_128x128_dgrad_wide", "dgrad", "bf16", (6, 128, 128, 65, 64, 3, 1, 1), SLAB % (BF, 128, 128, 1, 4)),
    # ---- conv3x3_slab_kernel, f32
    _c("slab_f32_128x64_fwd", "fwd", "f32", L1_ODD, SLAB % (FP, 128, 64, 0, 4)),
    _c("slab_f32_128x64_dgrad", "dgrad", "f32", L1_ODD, SLAB % (FP, 128, 64, 1, 4)),
    _c("slab_f32_128x64_dgrad_addend", "dgrad", "f32", (7, 256, 13, 11, 256, 3, 1, 1), SLAB % (FP, 128, 64, 1, 4), addend=True),
    _c("slab_f32_128x128_fwd", "fwd", "f32", (94, 64, 31, 17, 128, 3, 1, 1), SLAB % (FP, 128, 128, 0, 4)),
    _c("slab_f32_128x128_dgrad", "dgrad", "f32", (94, 128, 31, 17, 64, 3, 1, 1), SLAB % (FP, 128, 128, 1, 4)),
    # ---- conv_igemm_kernel: 3x3 stride 2 at even and odd sizes, 1x1 stride 2, the permuted stride-2 data gradient
    _c("flat_bf16_64_fwd_s2_even", "fwd", "bf16", S2_EVEN, flat(BF, 64, 64, 0)),
    _c("flat_bf16_64_dgrad_s2_even", "dgrad", "bf16", S2_EVEN, flat(BF, 64, 64, 1)),
    _c("flat_f32_64_fwd_s2_odd", "fwd", "f32", S2_ODD, flat(FP, 64, 64, 0)),
    _c("flat_f32_64_dgrad_s2_odd", "dgrad", "f32", S2_ODD, flat(FP, 64, 64, 1)),
    _c("flat_bf16_64_fwd_s2_odd", "fwd", "bf16", S2_ODD, flat(BF, 64, 64, 0)),
    _c("flat_bf16_64_dgrad_s2_odd", "dgrad", "bf16", S2_ODD, flat(BF, 64, 64, 1)),
    _c("flat_bf16_64_dgrad_s2_addend", "dgrad", "bf16", S2_ODD, flat(BF, 64, 64, 1), r=2, addend=True),
    _c("flat_bf16_128_fwd_s2_odd", "fwd", "bf16", (14, 64, 65, 47, 128, 3, 2, 1), flat(BF, 128, 64, 0)),
    _c("flat_bf16_128_dgrad_s2_odd", "dgrad", "bf16", (8, 64, 65, 47, 128, 3, 2, 1), flat(BF, 128, 64, 1)),
    _c("flat_bf16_256_fwd_s2_odd", "fwd", "bf16", (27, 64, 65, 47, 128, 3, 2, 1), flat(BF, 256, 64, 0)),
    _c("flat_bf16_256_dgrad_s2_odd", "dgrad", "bf16", (14, 64, 65, 47, 128, 3, 2, 1), flat(BF, 256, 64, 1)),
    _c("flat_f32_128_fwd_s2_odd", "fwd", "f32", (14, 64, 65, 47, 128, 3, 2, 1), flat(FP, 128, 64, 0)),
    _c("flat_f32_128_dgrad_s2_odd", "dgrad", "f32", (8, 64, 65, 47, 128, 3, 2, 1), flat(FP, 128, 64, 1)),
    _c("flat_f32_256_fwd_s2_odd", "fwd", "f32", (27, 64, 65, 47, 128, 3, 2, 1), flat(FP, 256, 64, 0)),
    _c("flat_f32_256_dgrad_s2_odd", "dgrad", "f32", (14, 64, 65, 47, 128, 3, 2, 1), flat(FP, 256, 64, 1)),
    _c("flat_bf16_64_fwd_1x1", "fwd", "bf16", (2, 64, 9, 6, 128, 1, 2, 0), flat(BF, 64, 64, 0)),
    _c("flat_bf16_64_dgrad_1x1", "dgrad", "bf16", (2, 64, 9, 6, 128, 1, 2, 0), flat(BF, 64, 64, 1)),
    _c("flat_bf16_128_fwd_1x1_odd", "fwd", "bf16", (14, 64, 65, 47, 128, 1, 2, 0), flat(BF, 128, 64, 0)),
    _c("flat_bf16_256_dgrad_1x1_odd", "dgrad", "bf16", (14, 64, 65, 47, 128, 1, 2, 0), flat(BF, 256, 64, 1)),
    _c("flat_f32_64_fwd_1x1", "fwd", "f32", (2, 64, 9, 6, 128, 1, 2, 0), flat(FP, 64, 64, 0)),
    _c("flat_bf16_64_dgrad_bn_s2", "dgrad_bn", "bf16", S2_ODD, flat(BF, 64, 64, 1), bits=True),   # F32ST: r = 1
    _c("flat_bf16_64_dgrad_relu_s2", "dgrad_relu", "bf16", S2_EVEN, flat(BF, 64, 64, 1), r=2),
    _c("flat_f32_64_dgrad_relu_1x1", "dgrad_relu", "f32", (2, 64, 9, 6, 128, 1, 2, 0), flat(FP, 64, 64, 1)),
    # gdl_conv_dgrad_ds: n = 9 K + K
    _c("ds_bf16_odd", "dgrad_ds", "bf16", S2_ODD, flat(BF, 64, 64, 1)),
    _c("ds_bf16_odd_bits", "dgrad_ds", "bf16", S2_ODD, flat(BF, 64, 64, 1), bits=True),
    _c("ds_bf16_256_odd_bits", "dgrad_ds", "bf16", (14, 64, 65, 47, 128, 3, 2, 1), flat(BF, 256, 64, 1), bits=True),
    _c("ds_f32_even", "dgrad_ds", "f32", S2_EVEN, flat(FP, 64, 64, 1)),
    _c("ds_f32_odd_bits", "dgrad_ds", "f32", S2_ODD, flat(FP, 64, 64, 1), bits=True),
    # the 128 x 128 plain-GEMM tile (y only)
    _c("flat_bf16_128x128_fwd_bias", "fwd_bias", "bf16", (1, 64, 181, 181, 128, 1, 1, 0), flat(BF, 128, 128, 0), r=2),
    # ---- split-K (the fold adds split - 1 fp32 additions: inside the ulp-per-addition charge)
    _c("split_fwd", "fwd_split", "bf16", (5, 512, 9, 6, 512, 3, 1, 1), SLAB % (BF, 128, 128, 0, 8)),
    # ---- the stem, n = 49 Cin: output rows of >= 64 pixels (persistent) and below (flat)
    _c("stem_bf16_pers_odd_h", "stem", "bf16", (2, 1, 1, 9, 190), STEM_PERS),
    _c("stem_bf16_pers_rgb", "stem", "bf16", (1, 3, 2, 7, 135), STEM_PERS),
    _c("stem_bf16_flat_audio", "stem", "bf16", (2, 1, 1, 65, 47), flat(BF, 64, 64, 0)),
    _c("stem_bf16_flat_rgb_odd", "stem", "bf16", (1, 3, 3, 33, 29), flat(BF, 64, 64, 0)),
    _c("stem_f32_wide", "stem", "f32", (2, 1, 1, 9, 190), flat(FP, 64, 64, 0)),
    _c("stem_f32_rgb_odd", "stem", "f32", (1, 3, 3, 33, 29), flat(FP, 64, 64, 0)),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# The kernels the list must reach (forward and data gradient): the 64-channel persistent kernel in its three instantiations, every
# persistent slab instantiation the planner can choose (a 192-row tile never has two slab buffers: 2 x 25 KiB and the kernel's
# 47 KiB of ring, staging and sums exceed the 96 KiB budget at any width), the slab kernel's bf16 tiles, its f32 tiles, the flat
# kernel's three tiles in both types, the plain-GEMM tile and the persistent stem.  The closing test of the GPU file compares the
# names the tap reported with this set.
REQUIRED_SLOTS = frozenset(
    [C64 % "0", C64 % "1", C64 % "1, true"]
    + [PS % (bm, mode, ns, 0) for bm, ns in ((192, 1), (128, 1), (128, 2)) for mode in (0, 1)]
    + [PS % (192, 1, 1, 1), PS % (128, 1, 1, 1), PS % (128, 1, 2, 1)]
    + [SLAB % (BF, bm, bn, mode, wv) for bm, bn, wv in ((128, 64, 4), (128, 128, 4), (192, 128, 4), (128, 128, 8)) for mode in (0, 1)]
    + [SLAB % (FP, 128, bn, mode, 4) for bn in (64, 128) for mode in (0, 1)]
    + [flat(t, bm, 64, mode) for t in (BF, FP) for bm in (64, 128, 256) for mode in (0, 1)]
    + [flat(BF, 128, 128, 0), STEM_PERS])
assert {c.slot for c in CASES} == REQUIRED_SLOTS, sorted({c.slot for c in CASES} ^ REQUIRED_SLOTS)

OLD_LIMIT = {"fwd": 3e-3, "dgrad": 4e-3}  # the norm-wise bf16 limits of tests/test_ops_gpu.py


def quant(a, dt):
    return cr.bf16_round(a) if dt == "bf16" else np.ascontiguousarray(a, dtype=np.float32)


def out_hw(shape):
    N, C, H, W, K, R, stride, pad = shape
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def _loud_rows(a):
    """The last pixel row of image i and the first of image i + 1 at ten times the scale: a tap that leaks across an image
    boundary becomes a large error instead of a typical one."""
    a[..., 0, :] *= 10.0
    a[..., -1, :] *= 10.0
    return a


def make_inputs(case):
    """Seeded Gaussian inputs of a case, quantised to its storage type (float32 numpy, NCHW)."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    dt, o = case.dt, case.opt
    g = lambda *s: rng.standard_normal(s, dtype=np.float32)
    if case.op == "stem":
        B, Cin, T, H, W = case.shape
        return {"x": quant(_loud_rows(g(B, Cin, T, H, W)), dt), "w": quant(g(64, Cin, 7, 7) * 0.1, dt)}
    N, C, H, W, K, R, stride, pad = case.shape
    P, Q = out_hw(case.shape)
    inp = {"w": quant(g(K, C, R, R) * np.float32(np.sqrt(2.0 / (C * R * R))), dt)}
    if case.op in ("fwd", "fwd_bias", "fwd_split"):
        inp["x"] = quant(_loud_rows(g(N, C, H, W)), dt)
        if case.op == "fwd_bias":
            inp["bias"] = g(K)
            inp["res"] = quant(g(N, K, P, Q), dt)
        return inp
    inp["dy"] = quant(_loud_rows(g(N, K, P, Q)), dt)
    if case.op == "dgrad_ds":
        inp["dy_ds"] = quant(_loud_rows(g(N, K, P, Q)), dt)
        inp["w_ds"] = quant(g(K, C, 1, 1) * np.float32(0.2), dt)
    if o.get("addend") or case.op == "dgrad_relu":
        inp["add"] = quant(g(N, C, H, W), dt)
    if o.get("bits") or case.op == "dgrad_relu":
        inp["keep"] = g(N, C, H, W) > 0
    if case.op == "dgrad_bn":
        inp["y1"] = quant(g(N, C, H, W) * np.float32(1.5) + np.float32(0.3), dt)
        inp["mean1"], inp["rstd1"] = g(C) * np.float32(0.3), (0.5 + rng.random(C)).astype(np.float32)
        if o.get("two"):
            inp["y2"] = quant(g(N, C, H, W), dt)
            inp["mean2"], inp["rstd2"] = g(C) * np.float32(0.3), (0.5 + rng.random(C)).astype(np.float32)
    return inp


def reduction_length(case):
    if case.op == "stem":
        return 49 * case.shape[1]
    N, C, H, W, K, R, stride, pad = case.shape
    if case.op in ("fwd", "fwd_bias", "fwd_split"):
        return R * R * C
    return R * R * K + (K if case.op == "dgrad_ds" else 0)


def reference(case, inp):
    """(ref64, bound, zero_where) of a case: conv_ref's float64 reference, its derived bound, the cleared ReLU bits."""
    if case.op == "stem":
        ref, mag = cr.stem_fwd(inp["x"], inp["w"])
    elif case.op in ("fwd", "fwd_bias", "fwd_split"):
        ref, mag = cr.conv_fwd(inp["x"], inp["w"], case.shape[6], case.shape[7])
    else:
        N, C, H, W, K, R, stride, pad = case.shape
        if case.op == "dgrad_ds":
            ref, mag = cr.conv_dgrad_ds(inp["dy"], inp["w"], inp["dy_ds"], inp["w_ds"], (H, W))
        elif stride == 1:
            ref, mag = cr.conv_dgrad_s1(inp["dy"], inp["w"], (H, W), pad)
        else:
            ref, mag = cr.conv_dgrad_s2(inp["dy"], inp["w"], (H, W), pad)
    extras = []
    if "add" in inp:
        extras.append(inp["add"].astype(np.float64))
    if case.op == "fwd_bias":
        extras += [inp["bias"].astype(np.float64)[None, :, None, None], inp["res"].astype(np.float64)]
    for e in extras:
        ref = ref + e
    bnd = cr.bound(ref, mag, reduction_length(case), cr.U_BF16 if case.dt == "bf16" else 0.0, case.r, extras)
    zero = None
    if "keep" in inp:
        zero = ~inp["keep"]
        ref = np.where(zero, 0.0, ref)
    return ref, bnd, zero


def fixture(case, inp):
    """What a correct kernel computes, on the CPU: torch float32 convolution of the quantised inputs (fp32 accumulation), the
    extras added in fp32, the ReLU mask, ONE rounding to the storage type.  float32 numpy, NCHW."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))

    def dgrad(dy, w, stride, pad, hw):
        P, Q, R = dy.shape[2], dy.shape[3], w.shape[2]
        op = (hw[0] - ((P - 1) * stride - 2 * pad + R), hw[1] - ((Q - 1) * stride - 2 * pad + R))
        return F.conv_transpose2d(t(dy), t(w), stride=stride, padding=pad, output_padding=op)

    if case.op == "stem":
        B, Cin, T, H, W = case.shape
        x4 = np.ascontiguousarray(np.transpose(inp["x"], (0, 2, 1, 3, 4))).reshape(B * T, Cin, H, W)
        out = F.conv2d(t(x4), t(inp["w"]), stride=2, padding=3)
    elif case.op in ("fwd", "fwd_bias", "fwd_split"):
        out = F.conv2d(t(inp["x"]), t(inp["w"]), stride=case.shape[6], padding=case.shape[7])
        if case.op == "fwd_bias":
            out = out + t(inp["bias"])[None, :, None, None] + t(inp["res"])
    else:
        N, C, H, W, K, R, stride, pad = case.shape
        out = dgrad(inp["dy"], inp["w"], stride, pad, (H, W))
        if case.op == "dgrad_ds":
            out = out + dgrad(inp["dy_ds"], inp["w_ds"], 2, 0, (H, W))
        if "add" in inp:
            out = out + t(inp["add"])
        if "keep" in inp:
            out = torch.where(t(inp["keep"].astype(np.float32)) > 0, out, torch.zeros(()))
    return quant(out.numpy(), case.dt)
