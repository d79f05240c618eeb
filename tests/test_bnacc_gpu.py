"""GPU tests, op level, of the kernels the default training step runs its BatchNorm work through and that only the encoder
reached so far: the integer-accumulator producers (convolution epilogues, csrc/bnacc.h bn_acc_add) and consumers
(bn_act_kernel<.., ACC>, bn_relu_maxpool_kernel<.., ACC>), the fused block backward (block_bwd_reduce_kernel, bn_bwd_apply2_kernel),
the paired finalizes and the accumulator clear of stem_pad_kernel.  Every comparison is element-wise or per-channel against
float64 (tests/bnacc_ref.py) or bit-for-bit against the unfused entry point; bounds are derived next to their use.  Each test
prints `RATIO <kernel> <dtype> <largest error / bound>`; docs/parity_log.md records the values of a run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnacc_ref as ref  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev, empty, gather_table, pack_weight, quant, to_nhwc  # noqa: E402

DTS = [L.GDL_F32, L.GDL_BF16]
U = 2.0 ** -24  # unit roundoff of float32
SLACK = 1.0 + 2.0 ** -20  # second-order terms of the first-order bounds below
EPS, MOM = 1e-5, 0.1
rng = np.random.default_rng(2025)


def _check_shape_list(name, shapes):
    """Collection-time guard (as in test_ops_gpu.py): every source line of the list carries exactly one tuple, in code -- a tuple
    that slipped into a trailing comment would silently never run."""
    import inspect
    import re
    import sys
    body = inspect.getsource(sys.modules[__name__]).split(name + " = [", 1)[1].split("\n]\n", 1)[0]
    code_rows = 0
    for ln in body.splitlines():
        code, _, comment = ln.partition("#")
        code_rows += code.count("(")
        assert not re.search(r"\(\s*\d+\s*,\s*\d+\s*,\s*\d+\s*,", comment), f"{name}: a shape tuple inside a comment: {ln.strip()}"
    assert code_rows == len(shapes), f"{name}: {code_rows} tuples in the source, {len(shapes)} parsed"


def _dtn(dt):
    return "bf16" if dt == L.GDL_BF16 else "f32"


def _record(kernel, dt, ratio):
    print(f"RATIO {kernel} {_dtn(dt)} {float(ratio):.3e}")


def _ratio(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max())


def _host(t):
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _half_ulp(x, dt):
    """half a unit in the last place of the storage type at magnitude x (0 for float32: the kernels store what they computed)"""
    if dt != L.GDL_BF16:
        return np.zeros_like(x)
    return 2.0 ** (np.floor(np.log2(np.maximum(x, 2.0 ** -126))) - 8)  # bf16: 8 significant bits


def _ulps(got32, want64):
    """|got - float32(want)| in units of float32(want)'s spacing; NaN where one is NaN and the other is not"""
    w32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    both_nan = np.isnan(got32) & np.isnan(w32)
    with np.errstate(invalid="ignore"):
        d = np.abs(got32.astype(np.float64) - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)
    return np.where(both_nan, 0.0, d)


# ------------------------------------------------------------------------------------------------ (a) producers
def _conv_case(N, C, H, W, K, R, dt, xscale=1.0):
    x = quant(rng.standard_normal((N, C, H, W), dtype=np.float32), dt) * np.float32(xscale)  # (a power of two: still exact)
    w = quant((rng.standard_normal((K, C, R, R), dtype=np.float32) * np.sqrt(2.0 / (C * R * R))).astype(np.float32), dt)
    return x, w


def _acc_words(K):
    return torch.zeros(2 * K + 1, dtype=torch.int64, device=DEV)  # [K][2] + the flag word, zeroed


def _conv_both_ways(shape, dt, xscale=1.0, split=False):
    """one launch with partial rows, two launches of the _acc entry (each into a fresh zeroed buffer) on the same inputs"""
    N, C, H, W, K, R, stride, pad = shape
    lib = L.load()
    st = L.cur_stream()
    x, w = _conv_case(N, C, H, W, K, R, dt, xscale)
    P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    xd = to_nhwc(x, dt)
    krsc, _ = pack_weight(w, dt)
    tab = gather_table(L.GATHER_FWD, dt, N, H, W, C, K, R, R, stride, pad)
    tiles = lib.gdl_conv_bn_tiles(dt, N, H, W, C, K, R, R, stride, pad)
    geom = (N, H, W, C, K, R, R, stride, pad)
    ws = None
    if split:
        need = lib.gdl_conv_split_workspace_bytes(dt, *geom, 0)
        assert need > 0, "this shape is expected to split"
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    y0 = empty((N, P, Q, K), dt)
    part = torch.full((tiles, K, 2), float("nan"), device=DEV)
    if split:
        L.call("gdl_conv_fwd_split", dt, L.ptr(xd), L.ptr(krsc), L.ptr(y0), L.ptr(part), L.ptr(tab), *geom, L.ptr(ws), ws.numel(), st)
    else:
        L.call("gdl_conv_fwd", dt, L.ptr(xd), L.ptr(krsc), L.ptr(y0), L.ptr(part), L.ptr(tab), *geom, st)
    runs = []
    for _ in range(2):
        y, acc = empty((N, P, Q, K), dt), _acc_words(K)
        L.call("gdl_conv_fwd_acc", dt, L.ptr(xd), L.ptr(krsc), L.ptr(y), L.ptr(acc), L.ptr(tab), *geom, L.ptr(ws),
               ws.numel() if split else 0, st)
        runs.append((y, acc))
    torch.cuda.synchronize()
    return y0, part, runs, N * P * Q


def _check_producer(y0, part, runs, rows, K):
    """y bit-identical between the two modes; the accumulator words EXACTLY the rounded partial rows, summed as integers -- `sacc`
    is a run-time field of one kernel instantiation in every epilogue family (conv_igemm.hip tile_sums, the two persistent
    epilogues, the split-K finish kernel, conv_pslab.h fold4): the float a tile stores as its partial row is the float
    bn_acc_add converts, so there is no summation-order term to allow for; flag word 0; a second launch gives the same words."""
    (y1, acc1), (y2, acc2) = runs
    assert _bits_equal(y1, y0) and _bits_equal(y2, y0)
    s1, s2 = ref.scales(rows)
    p = part.cpu().numpy()
    assert np.isfinite(p).all()
    want = ref.acc_from_partials(p, s1, s2)
    got = acc1.cpu().numpy()
    np.testing.assert_array_equal(got[:2 * K].reshape(K, 2), want)
    assert got[2 * K] == 0
    assert torch.equal(acc1, acc2)
    assert np.abs(want[:, 1]).min() > 0  # (every channel received its sums: an all-zero row would compare equal trivially)


PRODUCER_SHAPES = [
    # N, C, H, W, K, R, stride, pad       -> epilogue family
    (2, 64, 9, 6, 128, 1, 2, 0),      # flat kernel, 1x1 stride 2
    (3, 64, 20, 18, 128, 3, 2, 1),    # flat kernel, 3x3 stride 2
    (2, 64, 17, 13, 64, 3, 1, 1),     # slab kernel with a ragged tail
    (7, 256, 13, 11, 256, 3, 1, 1),   # slab kernel, two N-tiles, ragged last tile
    (24, 128, 17, 12, 128, 3, 1, 1),  # persistent slab kernel
    (3, 64, 65, 47, 64, 3, 1, 1),     # 64-channel persistent kernel, odd dims
    (2, 64, 33, 157, 64, 3, 1, 1),    # the same in its one-buffer form
    (8, 128, 14, 14, 384, 3, 1, 1),   # the 8-wave tile, three N-tiles
]
_check_shape_list("PRODUCER_SHAPES", PRODUCER_SHAPES)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", PRODUCER_SHAPES)
def test_conv_producer_exact(shape, dt):
    y0, part, runs, rows = _conv_both_ways(shape, dt)
    _check_producer(y0, part, runs, rows, shape[4])


def test_conv_split_k_producer_exact():
    """the split-K finish kernel's epilogue (bf16 only), ragged last M-tile"""
    N, C, H, W, K = 5, 512, 9, 6, 512
    y0, part, runs, rows = _conv_both_ways((N, C, H, W, K, 3, 1, 1), L.GDL_BF16, split=True)
    _check_producer(y0, part, runs, rows, K)


STEM_CASES = [
    # name, B, Cin, T, H, W
    ("visual_odd", 1, 3, 3, 33, 29),
    ("row64", 1, 3, 2, 12, 128),
]
_check_shape_list("STEM_CASES", STEM_CASES)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_producer_exact(case, dt):
    _, B, Cin, T, H, W = case
    lib = L.load()
    st = L.cur_stream()
    x = rng.standard_normal((B, Cin, T, H, W), dtype=np.float32)
    w = (rng.standard_normal((64, Cin, 7, 7), dtype=np.float32) * 0.1).astype(np.float32)
    n_img, P, Q = B * T, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.empty(lib.gdl_stem_pad_bytes(dt, n_img, H, W), dtype=torch.uint8, device=DEV)
    wp = torch.empty(lib.gdl_stem_weight_bytes(dt), dtype=torch.uint8, device=DEV)
    tab = torch.empty(lib.gdl_stem_table_bytes(n_img, H, W), dtype=torch.uint8, device=DEV)
    xd, wd = dev(x), dev(w)
    L.call("gdl_stem_pad", dt, L.ptr(xd), L.ptr(xp), B, Cin, T, H, W, st)
    L.call("gdl_pack_stem_rows", dt, L.ptr(wd), L.ptr(wp), Cin, st)
    L.call("gdl_stem_build_table", dt, n_img, H, W, L.ptr(tab), st)
    tiles = lib.gdl_stem_conv_bn_tiles(dt, n_img, H, W)
    y0 = empty((n_img, P, Q, 64), dt)
    part = torch.full((tiles, 64, 2), float("nan"), device=DEV)
    L.call("gdl_stem_conv_fwd", dt, L.ptr(xp), L.ptr(wp), L.ptr(y0), L.ptr(part), L.ptr(tab), n_img, H, W, Cin, st)
    runs = []
    for _ in range(2):
        y, acc = empty((n_img, P, Q, 64), dt), _acc_words(64)
        L.call("gdl_stem_conv_fwd_acc", dt, L.ptr(xp), L.ptr(wp), L.ptr(y), L.ptr(acc), L.ptr(tab), n_img, H, W, Cin, st)
        runs.append((y, acc))
    torch.cuda.synchronize()
    _check_producer(y0, part, runs, n_img * P * Q, 64)


def _publish_buffers(C):
    return [torch.full((C,), 7.0, device=DEV) for _ in range(4)]  # save_mean, save_rstd, scale, shift


@pytest.mark.parametrize("shape,dt", [((2, 64, 9, 6, 128, 1, 2, 0), L.GDL_F32), ((2, 64, 9, 6, 128, 1, 2, 0), L.GDL_BF16),
                                      ((24, 128, 17, 12, 128, 3, 1, 1), L.GDL_BF16)])
def test_producer_guard(shape, dt):
    """Inputs scaled by 2^22 (large, finite: the factor of test_step_gpu.py::test_bn_accumulator_guard): the sums of squares
    leave the fixed-point range.  A block whose |sum * s| is not below 4.6e18 / gridDim.x adds nothing and sets the flag word, so
    no word may be a wrapped sum: every word equals the exact integer sum of the rounded partial rows that pass ONE common
    threshold.  gridDim.x is not part of the C ABI; it is an integer, at least the number of partial rows (every row is written by
    a block of its own) and at most M-tiles x N-tiles rounded up to a multiple of 8 (common.h xcd_grid; an N-tile is at least 64
    channels wide, and a persistent kernel's rows ARE its blocks) -- the words must match for some
    integer in that range.  The consumer then publishes NaN statistics."""
    K = shape[4]
    y0, part, runs, rows = _conv_both_ways(shape, dt, xscale=2.0 ** 22)
    (y1, acc1), (_, acc2) = runs
    assert _bits_equal(y1, y0) and torch.equal(acc1, acc2)
    p = part.cpu().numpy()
    assert np.isfinite(p).all()
    s1, s2 = ref.scales(rows)
    got = acc1.cpu().numpy()
    tiles = p.shape[0]
    match = [g for g in range(tiles, -(-(tiles * (K // 64)) // 8) * 8 + 1)
             if np.array_equal(ref.acc_from_partials(p, s1, s2, grid=g)[0], got[:2 * K].reshape(K, 2))]
    assert match, "the accumulator words are no threshold-selected sum of the rounded partial rows"
    assert ref.acc_from_partials(p, s1, s2, grid=match[0])[1] == 1 and got[2 * K] != 0
    passed = int(np.count_nonzero(got[:2 * K]))
    print(f"guard: {tiles} partial rows, {passed} non-zero words, block counts that reproduce the words: {match[0]}..{match[-1]}")
    # the consumer on these accumulators: NaN constants, loudly
    C = K
    g_d, b_d = dev(np.ones(C, np.float32)), dev(np.zeros(C, np.float32))
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    sm, sr, sc, sh = _publish_buffers(C)
    out = empty(tuple(y1.shape), dt)
    L.call("gdl_bn_act_acc", dt, L.ptr(y1), L.ptr(acc1), L.ptr(g_d), L.ptr(b_d), L.ptr(rm), L.ptr(rv), L.ptr(nbt), L.ptr(sm),
           L.ptr(sr), L.ptr(sc), L.ptr(sh), None, None, None, None, None, None, None, None, None, None, None, rows, EPS, MOM, 1,
           L.ptr(out), None, C, L.cur_stream())
    torch.cuda.synchronize()
    for t in (sm, sr, sc, sh, rm, rv):
        assert bool(torch.isnan(t).all())
    assert int(nbt.item()) == 1


# ------------------------------------------------------------------------------------------------ (b) bn_act with accumulators
def _host_acc(C, rows):
    """accumulator words chosen on the host (the consumer is tested alone): every third mean negative, channel 1 with variance
    exactly 0 (all values 0.5), channel 2 with a second moment below mean^2 (what tile roundings can leave: the clamp)"""
    s1, s2 = ref.scales(rows)
    mu = 2.0 * rng.standard_normal(C)
    mu[::3] = -np.abs(mu[::3]) - 0.25
    var = 0.1 + 3.9 * rng.random(C)
    s, q = np.rint(mu * rows * s1), np.rint((var + mu * mu) * rows * s2)
    s[1], q[1] = 0.5 * rows * s1, 0.25 * rows * s2
    s[2], q[2] = -1.25 * rows * s1, np.rint(1.5625 * rows * s2) - np.rint(1e-6 * rows * s2)
    acc = np.zeros(2 * C + 1, dtype=np.int64)
    acc[0:2 * C:2], acc[1:2 * C:2] = s.astype(np.int64), q.astype(np.int64)
    return acc


class _Bn:
    """one BatchNorm's host values and device buffers for an ACC consumer launch"""

    def __init__(self, C, rows):
        self.C, self.rows = C, rows
        self.acc = _host_acc(C, rows)
        self.gamma = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
        self.gamma[::7] *= -1
        self.beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
        self.rm = (0.05 * rng.standard_normal(C)).astype(np.float32)
        self.rv = (1 + 0.1 * rng.random(C)).astype(np.float32)
        self.acc_d = torch.from_numpy(self.acc).to(DEV)
        self.g_d, self.b_d, self.rm_d, self.rv_d = dev(self.gamma), dev(self.beta), dev(self.rm), dev(self.rv)
        self.nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        self.sm, self.sr, self.sc, self.sh = _publish_buffers(C)

    def args(self):
        return [L.ptr(t) for t in (self.acc_d, self.g_d, self.b_d, self.rm_d, self.rv_d, self.nbt, self.sm, self.sr, self.sc, self.sh)]

    def check_published(self, kernel, dt, launches):
        """save_mean / save_rstd / scale / shift / running statistics against channel_constants, 1 ulp of float32: the device and
        numpy both evaluate in double, one rounding to float follows, and a last-bit difference of a double sqrt / division
        moves that rounding by at most one step.  The running statistics of launch n start from the float32 values launch
        n - 1 left: updated exactly once per launch however many blocks ran; num_batches_tracked rises by exactly 1."""
        s1, s2 = ref.scales(self.rows)
        k = ref.channel_constants(self.acc[:-1], 1.0 / s1, 1.0 / s2, self.rows, self.gamma, self.beta, EPS, MOM, self.rm, self.rv)
        self.rm, self.rv = _host(self.rm_d), _host(self.rv_d)  # (the next launch's start)
        worst = 0.0
        for name, got in (("mean", self.sm), ("rstd", self.sr), ("scale", self.sc), ("shift", self.sh),
                          ("running_mean", self.rm_d), ("running_var", self.rv_d)):
            d = _ulps(_host(got), k[name])
            assert d.max() <= 1.0, (kernel, name, int(d.argmax()), float(d.max()))
            worst = max(worst, float(d.max()))
        assert int(self.nbt.item()) == launches
        assert k["rstd"][1] == k["rstd"][2] == 1.0 / np.sqrt(float(np.float32(EPS)))  # variance 0 and the clamp
        _record(kernel + ":constants(ulp)", dt, worst)


ACT_SHAPES = [
    # M, C: chosen for the control flow of bn_act_kernel and ew_grid, not for size
    (3, 64),      # most threads are not live, yet all reach the barrier
    (40, 64),     # bf16: stride < nvec < 2 stride, pair is false for some threads
    (20, 64),     # f32: the same
    (1000, 64),   # four (bf16) / eight (f32) blocks: preloaded pair + loop trips + tail
    (37, 512),    # bf16: the constants loop runs twice per thread; f32: 128 vectors per row
    (2, 256),
]
_check_shape_list("ACT_SHAPES", ACT_SHAPES)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", ["none", "raw", "acc", "arrays"])
@pytest.mark.parametrize("shape", ACT_SHAPES)
def test_bn_act_acc(shape, mode, dt):
    """mode: the residual -- none | the raw tensor | res * rsc + rsf with the residual BatchNorm's accumulators | the same with
    finalized res_scale / res_shift arrays (RES == 2, fr.acc == nullptr).  ReLU + sign bits except with the raw residual."""
    M, C = shape
    epc = 8 if dt == L.GDL_BF16 else 4
    relu = mode != "raw"
    y = quant(rng.standard_normal((M, C), dtype=np.float32) * 1.5 + 0.2, dt)
    res = quant(rng.standard_normal((M, C), dtype=np.float32), dt)
    yd, rd = dev(y, L.torch_dtype(dt)), dev(res, L.torch_dtype(dt))
    bn = _Bn(C, M)
    rbn = _Bn(C, M) if mode == "acc" else None
    rsc0, rsf0 = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    rsc_d, rsf_d = dev(rsc0), dev(rsf0)
    if mode == "none":
        rargs = [None] * 11
    elif mode == "raw":
        rargs = [L.ptr(rd)] + [None] * 10
    elif mode == "acc":
        rargs = [L.ptr(rd)] + rbn.args()
    else:
        rargs = [L.ptr(rd)] + [None] * 8 + [L.ptr(rsc_d), L.ptr(rsf_d)]
    outs = []
    # (three launches: a block other than block 0 that published too would race with it on the running statistics, and shows
    # only when it reads what another block has already updated -- every launch of a multi-block shape is one more chance)
    for launch in (1, 2, 3):
        out = torch.full((M, C), 3.0, device=DEV).to(L.torch_dtype(dt))
        bits = torch.full((M * C // epc,), 0xA5, dtype=torch.uint8, device=DEV)
        L.call("gdl_bn_act_acc", dt, L.ptr(yd), *bn.args(), *rargs, M, EPS, MOM, 1 if relu else 0, L.ptr(out),
               L.ptr(bits) if relu else None, C, L.cur_stream())
        torch.cuda.synchronize()
        bn.check_published("bn_act_acc", dt, launch)
        if rbn:
            rbn.check_published("bn_act_acc", dt, launch)
        outs.append((out, bits))
    for o, b in outs[1:]:
        assert _bits_equal(outs[0][0], o) and torch.equal(outs[0][1], b)  # same accumulators, same constants
    out, bits = outs[0]
    # out element-wise against float64 with the PUBLISHED float32 constants.  fp32 evaluation, T1 = y sc, T2 = sf, T3 = res rsc
    # (or res), T4 = rsf: fl(T1) u|T1|; + T2: u(|T1| + |T2|); fl(T3) u|T3|; + T4: u(|T3| + |T4|); the final add
    # u(|T1| + |T2| + |T3| + |T4|): at most 3 u per term with a residual (k = 3), 2 u without (k = 2); a fused multiply-add
    # only drops roundings; ReLU is exact and 1-Lipschitz.  bf16 adds half an ulp of the result.
    sc, sf = _host(bn.sc).astype(np.float64), _host(bn.sh).astype(np.float64)
    y64, r64 = y.astype(np.float64), res.astype(np.float64)
    want, mag, k = y64 * sc[None, :] + sf[None, :], np.abs(y64 * sc[None, :]) + np.abs(sf)[None, :], 2
    if mode == "raw":
        want, mag, k = want + r64, mag + np.abs(r64), 3
    elif mode != "none":
        if mode == "acc":
            rsc, rsf = _host(rbn.sc).astype(np.float64), _host(rbn.sh).astype(np.float64)
        else:
            rsc, rsf = rsc0.astype(np.float64), rsf0.astype(np.float64)
            assert np.array_equal(_host(rsc_d), rsc0) and np.array_equal(_host(rsf_d), rsf0)  # read, not written
        want, mag, k = want + r64 * rsc[None, :] + rsf[None, :], mag + np.abs(r64 * rsc[None, :]) + np.abs(rsf)[None, :], 3
    if relu:
        want = np.maximum(want, 0.0)
    e32 = k * U * mag * SLACK
    bound = e32 + _half_ulp(np.abs(want) + e32, dt)
    got = _host(out).astype(np.float64)
    err = np.abs(got - want)
    assert np.all(err <= bound), (int((err / np.maximum(bound, 1e-300)).argmax()), _ratio(err, bound))
    _record("bn_act_acc:out", dt, _ratio(err, bound))
    if relu:  # every byte: the sign bits of the stored out
        g = (got.reshape(-1, epc) > 0).astype(np.int64)
        np.testing.assert_array_equal(bits.cpu().numpy(), (g << np.arange(epc)[None, :]).sum(1).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ (c) the stem's pool
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N,H,W", [(2, 33, 24), (3, 16, 16), (1, 7, 9)])
def test_bn_relu_maxpool_acc(N, H, W, dt):
    """out / idx / ymax bit-identical to gdl_bn_relu_maxpool_fwd fed the scale / shift the ACC launch published (every block
    derived the same constants block 0 published); the published constants as for bn_act."""
    C = 64
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = quant(rng.standard_normal((N, H, W, C), dtype=np.float32) * 1.5 + 0.2, dt)
    yd = dev(y, L.torch_dtype(dt))
    bn = _Bn(C, N * H * W)
    st = L.cur_stream()

    def bufs():
        return (torch.full((N, P, Q, C), 3.0, device=DEV).to(L.torch_dtype(dt)), torch.full((N, P, Q, C), 77, dtype=torch.uint8, device=DEV),
                torch.full((N, P, Q, C), 3.0, device=DEV).to(L.torch_dtype(dt)))

    o1, i1, m1 = bufs()
    L.call("gdl_bn_relu_maxpool_fwd_acc", dt, L.ptr(yd), *bn.args(), EPS, MOM, L.ptr(o1), L.ptr(i1), L.ptr(m1), N, H, W, C, st)
    torch.cuda.synchronize()
    bn.check_published("bn_relu_maxpool_acc", dt, 1)
    o2, i2, m2 = bufs()
    L.call("gdl_bn_relu_maxpool_fwd", dt, L.ptr(yd), L.ptr(bn.sc), L.ptr(bn.sh), L.ptr(o2), L.ptr(i2), L.ptr(m2), N, H, W, C, st)
    torch.cuda.synchronize()
    assert _bits_equal(o1, o2) and torch.equal(i1, i2) and _bits_equal(m1, m2)
    assert int(i1.max().item()) <= 8


# ------------------------------------------------------------------------------------------------ (d) block backward reduce
BWD_SHAPES = [
    # M, C
    (189, 64),
    (408, 128),   # four blocks
    (50, 256),
    (24, 512),
    (3000, 128),  # 24 blocks
]
_check_shape_list("BWD_SHAPES", BWD_SHAPES)


def _stats(C):
    return (0.3 * rng.standard_normal(C)).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ds,pre", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_block_bwd_reduce(shape, ds, pre, dt):
    M, C = shape
    tdt = L.torch_dtype(dt)
    dz, z, y2, yd = (quant(rng.standard_normal((M, C), dtype=np.float32), dt) for _ in range(4))
    (mean2, rstd2), (meand, rstdd) = _stats(C), _stats(C)
    dz_d, z_d, y2_d, yd_d = (dev(a, tdt) for a in (dz, z, y2, yd))
    m2_d, r2_d, md_d, rd_d = dev(mean2), dev(rstd2), dev(meand), dev(rstdd)
    blocks = L.load().gdl_bn_bwd_blocks(M, C)
    runs = []
    for _ in range(2):
        do2 = torch.full((M, C), 5.0, device=DEV).to(tdt)  # (a canary when premasked)
        p2 = torch.full((blocks, C, 2), float("nan"), device=DEV)
        pd = torch.full((blocks, C, 2), float("nan"), device=DEV)
        L.call("gdl_block_bwd_reduce", dt, L.ptr(dz_d), None if pre else L.ptr(z_d), L.ptr(y2_d), L.ptr(yd_d) if ds else None,
               L.ptr(m2_d), L.ptr(r2_d), L.ptr(md_d) if ds else None, L.ptr(rd_d) if ds else None, L.ptr(do2), L.ptr(p2),
               L.ptr(pd) if ds else None, M, C, 1 if pre else 0, L.cur_stream())
        torch.cuda.synchronize()
        runs.append((do2, p2, pd))
    do2, p2, pd = runs[0]
    assert _bits_equal(runs[1][1], p2) and (not ds or _bits_equal(runs[1][2], pd))  # two launches: identical partial rows
    if pre:
        assert bool((do2.float() == 5.0).all())  # not written
    else:
        assert _bits_equal(do2, torch.where(z_d > 0, dz_d, torch.zeros_like(dz_d)))
    _, s2, sd, a2, ad = ref.block_bwd_reduce(dz, z, y2, yd if ds else None, mean2, rstd2, meand, rstdd, pre)
    # Per channel the kernel adds n = M terms in float32 in SOME order (threads, then row-lanes; the blocks' rows are added here
    # in float64): any order of n float32 additions is within (n - 1) u sum|terms| of the exact sum; the issue's form of the
    # bound also grants one u per block.  A term of the second sum, g ((y - mean) rstd), carries three roundings (the
    # subtraction, two products): 3 u |term| more.  First sum: the terms are the stored values themselves.
    k = np.array([M - 1 + blocks, M - 1 + blocks + 3], dtype=np.float64)[None, :]
    for name, p, s, a in (("partial2", p2, s2, a2),) + ((("partiald", pd, sd, ad),) if ds else ()):
        got = p.double().sum(0).cpu().numpy()
        bound = k * U * a * SLACK
        err = np.abs(got - s)
        assert np.all(err <= bound), (name, _ratio(err, bound))
        _record("block_bwd_reduce:" + name, dt, _ratio(err, bound))
    if ds:
        assert _bits_equal(pd[..., 0], p2[..., 0])  # the sum of do2 is shared by both BatchNorms
        assert not _bits_equal(pd[..., 1], p2[..., 1])
    else:
        assert bool(torch.isnan(pd).all())


# ------------------------------------------------------------------------------------------------ (e) the two-sided apply
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_bn_bwd_apply2(shape, dt):
    """dy = gr (g - k1 - (y - mean) rstd k2), gr = fl(gamma rstd), per side (bn.hip bn_bwd_apply2_kernel).  Roundings: a = y - mean,
    b = a rstd, c = b k2: |dc| <= 3 u |c|; d = g - k1: u (|g| + |k1|); e = d - c: |de| <= |dd| + |dc| + u |e| <= u (2 |g| + 2 |k1| +
    4 |c|); gr and the last product add 2 u |e|: |d dy| <= |gamma rstd| u (4 |g| + 4 |k1| + 6 |c|) <= 6 u |gamma rstd| (|g| + |k1| +
    |c|) -- k = 6; a fused multiply-add only drops roundings.  bf16 adds half an ulp of the result.  Different gamma / mean /
    rstd / coef and a different y per side: exchanged sides cannot pass."""
    M, C = shape
    tdt = L.torch_dtype(dt)
    g, yA, yB = (quant(rng.standard_normal((M, C), dtype=np.float32), dt) for _ in range(3))
    (meanA, rstdA), (meanB, rstdB) = _stats(C), _stats(C)
    gammaA, gammaB = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32), (-1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    coefA, coefB = (0.2 * rng.standard_normal((2, C))).astype(np.float32), (0.2 * rng.standard_normal((2, C))).astype(np.float32)
    g_d, yA_d, yB_d = (dev(a, tdt) for a in (g, yA, yB))
    side = [[dev(a) for a in (meanA, rstdA, gammaA, coefA)], [dev(a) for a in (meanB, rstdB, gammaB, coefB)]]
    dA, dB = torch.full((M, C), 5.0, device=DEV).to(tdt), torch.full((M, C), 5.0, device=DEV).to(tdt)
    L.call("gdl_bn_bwd_apply2", dt, L.ptr(g_d), L.ptr(yA_d), *[L.ptr(t) for t in side[0]], L.ptr(dA), L.ptr(yB_d),
           *[L.ptr(t) for t in side[1]], L.ptr(dB), M, C, L.cur_stream())
    torch.cuda.synchronize()
    (wA, magA), (wB, magB) = ref.bn_bwd_apply2(g, yA, meanA, rstdA, gammaA, coefA, yB, meanB, rstdB, gammaB, coefB)
    worst = 0.0
    for name, got, want, mag in (("dyA", dA, wA, magA), ("dyB", dB, wB, magB)):
        e32 = 6 * U * mag * SLACK
        bound = e32 + _half_ulp(np.abs(want) + e32, dt)
        err = np.abs(_host(got).astype(np.float64) - want)
        assert np.all(err <= bound), (name, _ratio(err, bound))
        worst = max(worst, _ratio(err, bound))
    _record("bn_bwd_apply2", dt, worst)


# ------------------------------------------------------------------------------------------------ (f) paired finalizes
@pytest.mark.parametrize("C", [64, 128, 256, 512])  # every fin_ch value: 1, 2, 4, 8 channels per block
def test_paired_finalizes_bit_identical_to_single_launches(C):
    st = L.cur_stream()
    tiles = (7, 300)  # different row counts on the two sides; 300: more rows than row-lanes at every width
    counts = [float(t * 16 + 3) for t in tiles]
    parts, gam, bet = [], [], []
    for t in tiles:
        p = np.empty((t, C, 2), np.float32)
        p[..., 0] = 8.0 * rng.standard_normal((t, C))
        p[..., 1] = 16.0 * (1.0 + rng.random((t, C)))
        parts.append(dev(p))
        gam.append(dev((1 + 0.3 * rng.standard_normal(C)).astype(np.float32)))
        bet.append(dev((0.2 * rng.standard_normal(C)).astype(np.float32)))
    rm0 = [(0.05 * rng.standard_normal(C)).astype(np.float32) for _ in tiles]
    rv0 = [(1 + 0.1 * rng.random(C)).astype(np.float32) for _ in tiles]

    def train_bufs(i):
        return [dev(rm0[i]), dev(rv0[i]), torch.full((), 4, dtype=torch.int64, device=DEV)] + _publish_buffers(C)

    single = [train_bufs(0), train_bufs(1)]
    for i in range(2):
        L.call("gdl_bn_finalize_train", L.ptr(parts[i]), tiles[i], C, counts[i], L.ptr(gam[i]), L.ptr(bet[i]), EPS, MOM,
               *[L.ptr(t) for t in single[i]], st)
    pair = [train_bufs(0), train_bufs(1)]
    args = []
    for i in range(2):
        args += [L.ptr(parts[i]), tiles[i], counts[i], L.ptr(gam[i]), L.ptr(bet[i])] + [L.ptr(t) for t in pair[i]]
    L.call("gdl_bn_finalize_train_pair", *args, C, EPS, MOM, st)
    torch.cuda.synchronize()
    for i in range(2):
        for a, b in zip(single[i], pair[i]):
            assert _bits_equal(a, b)
        assert int(pair[i][2].item()) == 5 and bool(torch.isfinite(pair[i][4]).all())
    assert not _bits_equal(pair[0][3], pair[1][3])  # (the two sides are different BatchNorms)

    def bwd_bufs():
        return [torch.full((C,), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV), torch.full((2 * C,), 7.0, device=DEV)]

    single = [bwd_bufs(), bwd_bufs()]
    for i in range(2):
        L.call("gdl_bn_bwd_finalize", L.ptr(parts[i]), tiles[i], C, counts[i], *[L.ptr(t) for t in single[i]], st)
    pair = [bwd_bufs(), bwd_bufs()]
    args = []
    for i in range(2):
        args += [L.ptr(parts[i]), tiles[i], counts[i]] + [L.ptr(t) for t in pair[i]]
    L.call("gdl_bn_bwd_finalize_pair", *args, C, st)
    torch.cuda.synchronize()
    for i in range(2):
        for a, b in zip(single[i], pair[i]):
            assert _bits_equal(a, b) and not bool((b == 7.0).any())
    assert not _bits_equal(pair[0][2], pair[1][2])


# ------------------------------------------------------------------------------------------------ (g) the accumulator clear
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cin,W", [(1, 10), (3, 9)])  # padded width 18 / 17: bf16 takes its two-pixel / its one-pixel path
def test_stem_pad_zero(Cin, W, dt):
    """the padded image bit-identical to gdl_stem_pad's; the region all zero at 16 bytes, at a size below one grid pass (the
    image's 2 blocks x 256 threads x 16 bytes = 8 192) that crosses a block boundary, and at several passes plus a tail; 64
    canary bytes before and after untouched."""
    B, T, H = 1, 1, 10
    lib = L.load()
    st = L.cur_stream()
    n = lib.gdl_stem_pad_bytes(dt, B * T, H, W)
    assert -(-(B * T * (H + 6) * (W + 8)) // 256) == 2  # the grid the sizes below are chosen for
    x = dev(rng.standard_normal((B, Cin, T, H, W), dtype=np.float32))
    xp0 = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    L.call("gdl_stem_pad", dt, L.ptr(x), L.ptr(xp0), B, Cin, T, H, W, st)
    for zbytes in (16, 4112, 5 * 8192 + 48):
        buf = torch.full((64 + zbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        region = buf[64:64 + zbytes]
        assert region.data_ptr() % 16 == 0
        xp = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
        L.call("gdl_stem_pad_zero", dt, L.ptr(x), L.ptr(xp), B, Cin, T, H, W, L.ptr(region), zbytes, st)
        torch.cuda.synchronize()
        assert torch.equal(xp, xp0)
        assert int(region.count_nonzero().item()) == 0, zbytes
        assert bool((buf[:64] == 0xA5).all()) and bool((buf[64 + zbytes:] == 0xA5).all())
