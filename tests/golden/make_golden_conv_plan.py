"""Writes tests/golden/conv_plan.json: what the host-side convolution planner answers through the C ABI for a sweep
of geometries (tests/test_conv_plan_cpu.py asserts every value).  No GPU is needed: the queries are host code.

The committed fixture was recorded from a build of the PARENT of the commit that introduced `ConvGeom` (csrc/gather.h),
not from that commit's own build -- it pins the planner across the change of the internal interface from ten positional
integers to one struct, where the risk is a transposed field.  Re-record it only from a build whose planner is the
intended one, with no tuning variable set:

    GDL_LIB=/path/to/libgdl_hip.so python tests/golden/make_golden_conv_plan.py

This module is also the test's source of the sweep and of the query order (sweep(), query(), engine_bytes()).
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "conv_plan.json")

FIELDS = ("N", "H", "W", "C", "K", "R", "S", "stride", "pad")
DTYPES = ("bf16", "f32")
# one record per geometry and dtype, in this order
QUERIES = ("bn_tiles", "dgrad_bn_tiles", "table_bytes_fwd", "table_bytes_dgrad", "split_ws_fwd", "split_ws_dgrad", "wgrad_ws")

# the encoders' inputs of bench.py's workloads: (modality, T, H, W)
ENGINE_INPUTS = (
    ("audio", 1, 257, 188),   # cremad
    ("audio", 1, 129, 626),   # ks / vggsound / vggsound_swin: the wider audio maps
    ("visual", 3, 224, 224),  # every ResNet workload
)
BATCHES = (2, 64)

# geometries that tell the fields apart (the test states which one guards which pair of fields)
GUARDS = (
    (2, 56, 40, 64, 128, 3, 3, 2, 1),    # H != W, C != K, stride 2
    (2, 40, 56, 64, 128, 3, 3, 2, 1),
    (64, 28, 28, 128, 384, 3, 3, 1, 1),  # 128 -> 384: three N-tiles
    (64, 28, 28, 384, 128, 3, 3, 1, 1),
    (4, 14, 20, 256, 512, 3, 3, 1, 1),   # 256 -> 512, stride 1 against ...
    (4, 14, 20, 256, 512, 3, 3, 2, 1),   # ... stride 2
    (4, 14, 20, 256, 512, 1, 1, 1, 0),   # R = 1 against R = 3, pad 0 against pad 1
    (4, 14, 20, 256, 512, 1, 1, 2, 0),
    (4, 14, 20, 256, 512, 3, 1, 1, 1),   # R != S
    (4, 14, 20, 256, 512, 1, 3, 1, 1),
    (4, 3, 14, 256, 512, 1, 3, 1, 1),    # H = 3 beside R = 1, W = 3 beside S = 1: maps small enough to swap with the filter
    (4, 14, 3, 256, 512, 3, 1, 1, 1),
    (3, 33, 24, 128, 128, 3, 3, 1, 0),   # 3x3 without padding
    (192, 64, 128, 256, 320, 3, 3, 2, 1),  # N, H, W, C, K: five different multiples of 64
)


def resnet18_convs(n_img, H, W):
    """The 3x3 / 1x1 convolutions behind the stem of the ResNet18 encoder for an n_img x H x W input, in launch order."""
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1  # conv 7x7 / 2, pad 3
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1  # max-pool 3x3 / 2, pad 1
    out, cin = [], 64
    for li, planes in enumerate((64, 128, 256, 512)):
        for bk in range(2):
            stride = 2 if (bk == 0 and li > 0) else 1
            p, q = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
            out.append((n_img, h, w, cin, planes, 3, 3, stride, 1))
            out.append((n_img, p, q, planes, planes, 3, 3, 1, 1))
            if stride != 1 or cin != planes:
                out.append((n_img, h, w, cin, planes, 1, 1, stride, 0))
            cin, h, w = planes, p, q
    return out


def swin_linears(n_img):
    """The Linears of the Swin-T visual encoder (224 x 224, patch 4, embed 96, depths 2 2 6 2) as the 1x1 convolutions
    gdl/swin.py launches: M rows of kp -> np channels, every width padded to a multiple of 64."""
    ld = lambda c: -(-c // 64) * 64
    M, C = n_img * 56 * 56, 96
    out = [(M, 1, 1, ld(48), ld(C), 1, 1, 1, 0)]  # patch embedding
    for stage in range(4):
        out += [(M, 1, 1, ld(C), 3 * ld(C), 1, 1, 1, 0), (M, 1, 1, ld(C), ld(C), 1, 1, 1, 0),
                (M, 1, 1, ld(C), ld(4 * C), 1, 1, 1, 0), (M, 1, 1, ld(4 * C), ld(C), 1, 1, 1, 0)]
        if stage < 3:
            M //= 4
            out.append((M, 1, 1, ld(4 * C), ld(2 * C), 1, 1, 1, 0))  # patch merging
            C *= 2
    return out


def sweep():
    seen, out = set(), []
    geoms = []
    for B in BATCHES:
        for _, T, H, W in ENGINE_INPUTS:
            geoms += resnet18_convs(B * T, H, W)
        geoms += swin_linears(B * 3)
    for g in geoms + list(GUARDS):
        if g not in seen:
            seen.add(g)
            out.append(g)
    return out


def load():
    sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))
    from gdl import _lib as L

    return L, L.load()


def query(L, lib, dtype, g, wgrad=True):
    """The QUERIES for geometry g = FIELDS, as a list of integers (wgrad=False: without the last one, which has no answer
    for a channel count below one tile)."""
    dt = L.dtype_code(dtype)
    N, H, W, C, K, R, S, stride, pad = g
    return [lib.gdl_conv_bn_tiles(dt, *g), lib.gdl_conv_dgrad_bn_tiles(dt, *g),
            lib.gdl_conv_table_bytes(0, N, H, W, R, S, stride, pad), lib.gdl_conv_table_bytes(1, N, H, W, R, S, stride, pad),
            lib.gdl_conv_split_workspace_bytes(dt, *g, 0), lib.gdl_conv_split_workspace_bytes(dt, *g, 1)] + \
        ([lib.gdl_conv_wgrad_workspace_bytes(dt, *g)] if wgrad else [])


def engine_bytes(L, lib, modality, dtype, B, T, H, W):
    h = ctypes.c_void_p()
    L.call("gdl_encoder_create", ctypes.byref(h), L.GDL_AUDIO if modality == "audio" else L.GDL_VISUAL, L.dtype_code(dtype), B, T, H, W)
    try:
        return lib.gdl_encoder_workspace_bytes(h)
    finally:
        lib.gdl_encoder_destroy(h)


def main():
    assert not os.environ.get("GDL_TUNING"), "record the fixture with the tuning variables unset"
    L, lib = load()
    convs = [{"g": list(g), **{dt: query(L, lib, dt, g) for dt in DTYPES}} for g in sweep()]
    engines = [{"modality": m, "dtype": dt, "B": B, "T": T, "H": H, "W": W, "bytes": engine_bytes(L, lib, m, dt, B, T, H, W)}
               for B in BATCHES for (m, T, H, W) in ENGINE_INPUTS for dt in DTYPES]
    with open(OUT, "w") as f:
        f.write('{"fields": %s,\n "queries": %s,\n "convs": [\n' % (json.dumps(FIELDS), json.dumps(QUERIES)))
        f.write(",\n".join("  " + json.dumps(c) for c in convs))
        f.write('\n ],\n "engines": [\n')
        f.write(",\n".join("  " + json.dumps(e) for e in engines))
        f.write("\n ]}\n")
    print(f"{OUT}: {len(convs)} geometries x {len(DTYPES)} dtypes, {len(engines)} engine shapes, library {L.SO_PATH}")


if __name__ == "__main__":
    main()
