"""Every planned convolution kernel, element by element: each case of tests/conv_cases.py runs through the C ABI as the
product runs it, with guard bands around every tensor, against conv_ref's float64 reference and per-element bound; a second
launch under the timing tap must name exactly the expected kernel slot and reproduce the first launch bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import conv_cases as cc
import conv_ref as cr

pytestmark = pytest.mark.gpu

from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev, gather_table  # noqa: E402

HELPER_SLOTS = {"gdl::splitk_finish_kernel"}  # launches beside the convolution kernel that a case may make
SEEN = {}                                      # case id -> the slot the tap reported (the closing test reads it)


def _sync():
    """Device synchronisation; a device error here (a fault of the launch just made) ends the session: nothing more is started on a
    device that faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after a convolution launch: {e}", returncode=3)


def _code(case):
    return L.GDL_BF16 if case.dt == "bf16" else L.GDL_F32


def _g_in(a_nchw, tdt):
    """NCHW float32 numpy -> guarded NHWC device tensor of the storage type, NaN bands."""
    t = torch.from_numpy(np.ascontiguousarray(a_nchw, dtype=np.float32)).to(DEV).permute(0, 2, 3, 1).contiguous().to(tdt)
    return cr.guarded(tuple(t.shape), tdt, "nan", DEV, fill=t)


def _g_vec(a, dtype=torch.float32):
    t = dev(a, dtype)
    return cr.guarded(tuple(t.shape), dtype, "nan", DEV, fill=t)


def _bits(keep_nchw, epc):
    kb = np.ascontiguousarray(np.transpose(keep_nchw, (0, 2, 3, 1))).reshape(-1, epc)
    return (kb * (1 << np.arange(epc))[None, :]).sum(1).astype(np.uint8)


def _tap_counts(lib):
    ns = lib.gdl_prof_nslots()
    n_l, n_ms, n_w = (ctypes.c_int64 * max(ns, 1))(), (ctypes.c_double * max(ns, 1))(), (ctypes.c_double * max(ns, 1))()
    L.call("gdl_prof_collect", n_l, n_ms, n_w)
    out = {}
    for s in range(ns):
        if n_l[s]:
            name = lib.gdl_prof_slot_name(s)
            out[name.decode() if isinstance(name, bytes) else name] = int(n_l[s])
    return out


def _prepare(case, inp):
    """Device state of a case: guarded inputs, packed weights, tables.  Returns (launch, out_shape_nhwc, fill, checks):
    launch(out) enqueues the case's launch writing `out`; fill is the addend an in-place launch starts from (or None)."""
    lib = L.load()
    dt, tdt, st = _code(case), L.torch_dtype(_code(case)), L.cur_stream()
    epc = 8 if case.dt == "bf16" else 4
    checks, keep_alive = [], []

    def gin(a):
        v, chk = _g_in(a, tdt)
        checks.append(chk)
        return v

    def gvec(a, dtype=torch.float32):
        v, chk = _g_vec(a, dtype)
        checks.append(chk)
        return v

    def scratch(shape, dtype=torch.float32):  # statistics rows and other side outputs: NaN-filled, guarded
        v, chk = cr.guarded(shape, dtype, "pattern", DEV)
        checks.append(chk)
        return v

    if case.op == "stem":
        B, Cin, T, H, W = case.shape
        n_img, P, Q = B * T, (H - 1) // 2 + 1, (W - 1) // 2 + 1
        xp = torch.empty(lib.gdl_stem_pad_bytes(dt, n_img, H, W), dtype=torch.uint8, device=DEV)
        wp = torch.empty(lib.gdl_stem_weight_bytes(dt), dtype=torch.uint8, device=DEV)
        tab = torch.empty(lib.gdl_stem_table_bytes(n_img, H, W), dtype=torch.uint8, device=DEV)
        xd, wd = dev(inp["x"]), dev(inp["w"])
        L.call("gdl_stem_pad", dt, L.ptr(xd), L.ptr(xp), B, Cin, T, H, W, st)
        L.call("gdl_pack_stem_rows", dt, L.ptr(wd), L.ptr(wp), Cin, st)
        L.call("gdl_stem_build_table", dt, n_img, H, W, L.ptr(tab), st)
        part = scratch((lib.gdl_stem_conv_bn_tiles(dt, n_img, H, W), 64, 2))
        keep_alive += [xp, wp, tab, xd, wd]

        def launch(out):
            L.call("gdl_stem_conv_fwd", dt, L.ptr(xp), L.ptr(wp), L.ptr(out), L.ptr(part), L.ptr(tab), n_img, H, W, Cin, st)

        launch.keep = keep_alive
        return launch, (n_img, P, Q, 64), None, checks

    N, C, H, W, K, R, stride, pad = case.shape
    P, Q = cc.out_hw(case.shape)
    geo = (N, H, W, C, K, R, R, stride, pad)
    wd = dev(inp["w"])
    krsc, chk_k = cr.guarded((K, R, R, C), tdt, "nan", DEV)
    crsk, chk_c = cr.guarded((C, R, R, K), tdt, "nan", DEV)
    checks += [chk_k, chk_c]
    L.call("gdl_pack_weight", dt, L.ptr(wd), L.ptr(krsc), L.ptr(crsk), K, C, R, R, st)
    fwd = case.op in ("fwd", "fwd_bias", "fwd_split")
    tab = gather_table(L.GATHER_FWD if fwd else L.GATHER_DGRAD, dt, *geo)
    keep_alive += [wd, tab]
    fill = None
    if fwd:
        x = gin(inp["x"])
        if case.op == "fwd_bias":
            bias, res, ge = gvec(inp["bias"]), gin(inp["res"]), scratch((N, P, Q, K), tdt)

            def launch(out):
                L.call("gdl_conv_fwd_bias", dt, L.ptr(x), L.ptr(krsc), L.ptr(out), L.ptr(bias), L.ptr(res), L.ptr(ge), L.ptr(tab), *geo, st)
        else:
            part = scratch((lib.gdl_conv_bn_tiles(dt, *geo), K, 2))
            if case.op == "fwd_split":
                need = lib.gdl_conv_split_workspace_bytes(dt, *geo, 0)
                assert need > 0, "the split case is expected to split"
                ws = scratch((need,), torch.uint8)

                def launch(out):
                    L.call("gdl_conv_fwd_split", dt, L.ptr(x), L.ptr(krsc), L.ptr(out), L.ptr(part), L.ptr(tab), *geo, L.ptr(ws), need, st)
            else:
                def launch(out):
                    L.call("gdl_conv_fwd", dt, L.ptr(x), L.ptr(krsc), L.ptr(out), L.ptr(part), L.ptr(tab), *geo, st)
        launch.keep = keep_alive
        return launch, (N, P, Q, K), None, checks

    dy = gin(inp["dy"])
    bits = gvec(_bits(inp["keep"], epc), torch.uint8) if "keep" in inp else None
    if "add" in inp:
        fill = torch.from_numpy(inp["add"]).to(DEV).permute(0, 2, 3, 1).contiguous().to(tdt)
    if case.op == "dgrad":
        def launch(out):
            L.call("gdl_conv_dgrad", dt, L.ptr(dy), L.ptr(crsk), L.ptr(out), L.ptr(out) if fill is not None else None, L.ptr(tab), *geo, st)
    elif case.op == "dgrad_relu":
        def launch(out):
            L.call("gdl_conv_dgrad_relu", dt, L.ptr(dy), L.ptr(crsk), L.ptr(out), L.ptr(out), L.ptr(bits), L.ptr(tab), *geo, st)
    elif case.op == "dgrad_bn":
        two = bool(case.opt.get("two"))
        tiles = lib.gdl_conv_dgrad_bn_tiles(dt, *geo)
        y1, m1, r1, p1 = gin(inp["y1"]), gvec(inp["mean1"]), gvec(inp["rstd1"]), scratch((tiles, C, 2))
        y2, m2, r2, p2 = (gin(inp["y2"]), gvec(inp["mean2"]), gvec(inp["rstd2"]), scratch((tiles, C, 2))) if two else (None,) * 4

        def launch(out):
            L.call("gdl_conv_dgrad_bn", dt, L.ptr(dy), L.ptr(crsk), L.ptr(out), None, L.ptr(bits), L.ptr(tab), *geo, L.ptr(y1), L.ptr(m1),
                   L.ptr(r1), L.ptr(p1), L.ptr(y2), L.ptr(m2), L.ptr(r2), L.ptr(p2), st)
    else:
        assert case.op == "dgrad_ds"
        dyd = gin(inp["dy_ds"])
        wdsd = dev(inp["w_ds"])
        k11, chk1 = cr.guarded((K, 1, 1, C), tdt, "nan", DEV)
        ck, chk2 = cr.guarded((C, 1, 1, K), tdt, "nan", DEV)
        checks += [chk1, chk2]
        L.call("gdl_pack_weight", dt, L.ptr(wdsd), L.ptr(k11), L.ptr(ck), K, C, 1, 1, st)
        keep_alive += [wdsd]

        def launch(out):
            L.call("gdl_conv_dgrad_ds", dt, L.ptr(dy), L.ptr(crsk), L.ptr(dyd), L.ptr(ck), L.ptr(out), L.ptr(bits), L.ptr(tab), N, H, W, C,
                   K, st)
    launch.keep = keep_alive
    return launch, (N, H, W, C), fill, checks


@pytest.mark.parametrize("case", cc.CASES, ids=[c.id for c in cc.CASES])
def test_conv_elementwise(case):
    lib = L.load()
    tdt = L.torch_dtype(_code(case))
    inp = cc.make_inputs(case)
    ref64, bnd, zero = cc.reference(case, inp)
    launch, oshape, fill, checks = _prepare(case, inp)
    # 1. the launch as the product runs it: every element inside the bound, exact zeros under cleared ReLU bits, no band touched
    out1, chk1 = cr.guarded(oshape, tdt, "pattern", DEV, fill=fill)
    launch(out1)
    _sync()
    got = out1.float().permute(0, 3, 1, 2).contiguous().cpu().numpy()
    worst = cr.check(got, ref64, bnd, zero_where=zero)
    print(f"RATIO | {case.id} | {case.slot} | {worst:.3f}")
    chk1("(output)")
    for i, chk in enumerate(checks):
        chk(f"(operand {i})")
    # 2. the same launch under the timing tap: exactly the expected kernel served it, bit-identical result
    out2, chk2 = cr.guarded(oshape, tdt, "pattern", DEV, fill=fill)
    _tap_counts(lib)  # (clears records an earlier user of the tap may have left)
    lib.gdl_prof_enable(1)
    try:
        launch(out2)
        _sync()
        counts = _tap_counts(lib)
    finally:
        lib.gdl_prof_enable(0)
    kernels = {k: v for k, v in counts.items() if k not in HELPER_SLOTS}
    SEEN[case.id] = sorted(kernels)
    assert kernels == {case.slot: 1}, f"{case.id}: expected one launch of {case.slot}, the tap counted {counts}"
    chk2("(output, second launch)")
    assert torch.equal(out1.view(torch.uint8), out2.view(torch.uint8)), "second launch differs from the first"


def test_case_list_reaches_every_required_kernel():
    """The union of the slots the tap reported equals the required kernels (conv_cases.REQUIRED_SLOTS).  With the whole list run the
    comparison is over the reported names; a run that deselected cases can only check the names it has."""
    assert {c.slot for c in cc.CASES} == cc.REQUIRED_SLOTS
    seen = {s for names in SEEN.values() for s in names}
    assert seen <= cc.REQUIRED_SLOTS, sorted(seen - cc.REQUIRED_SLOTS)
    if set(SEEN) == set(cc.BY_ID):
        assert seen == cc.REQUIRED_SLOTS, sorted(cc.REQUIRED_SLOTS - seen)
