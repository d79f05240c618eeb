"""Float64 references, a derived per-element error bound and a checker for the convolution kernels (CPU only: numpy and
torch CPU in float64).  tests/test_conv_ref_cpu.py tests this module itself, tests/test_conv_elementwise_gpu.py uses it on
the kernels, tests/conv_cases.py is the case list both share.

Reference functions.  Each returns (ref64, mag), NCHW float64: `ref64` is the exact result from the already-quantised
inputs, `mag` the same contraction of |input| and |weight| -- the sum of the absolute products per output element.

The bound per output element.  A kernel multiplies storage-type inputs (bf16 x bf16 products are exact in fp32), accumulates
n = R*S*IC products in fp32 in SOME order (the matrix core's, the K-loop's, split-K's fold), adds the extras (addend, bias,
residual) and rounds to the storage type.  With eps = 2^-24 (half an fp32 ulp, relative):

    acc   = 2 * (n + 1) * eps * mag  +  2 * eps * |extras|

charges ONE fp32 ulp (2 eps) per addition where round-to-nearest costs half: every partial sum of an n-term sum is at most mag,
n - 1 additions and the n products (exact for bf16, one rounding each for f32) make < n + 1 roundings of at most mag each
-- any summation order stays below it (Higham, Accuracy and Stability, 4.2, with gamma_n ~ n u), and the doubled unit
leaves room for hardware that truncates internally.  |extras| is the sum of the absolute extras, each added once.

    bound = acc + u_out * (|ref64| + acc)                       r = 1
          + u_out * (|ref64 - extras| + acc)                    r = 2 (a rounding BEFORE the extras are added)

u_out is the unit roundoff of the storage type, 2^-8 for bf16 (8 significand bits, round to nearest) and 0 for f32.  The
value a rounding acts on is within acc of the exact one, hence (|exact| + acc).  r is the number of roundings to the
storage type on the path, READ FROM THE EPILOGUE CODE (never from results) and stated beside each case:
  * conv_epilogue (flat and slab kernels), conv3x3_pslab_kernel, conv3x3_c64_kernel without BatchNorm sums and
    splitk_finish_kernel stage the accumulators through LDS as the storage type; a launch with an addend or a bias
    unpacks that value, adds in fp32 and packs again: r = 2 with extras, 1 without.  The first rounding acts on the
    contraction alone, ref64 - extras, which an addend of opposite sign leaves far larger than |ref64|: charging it as
    u_out * |ref64| would not be a bound.  Without extras the two terms are equal and the sum is r * u_out * (|ref64| + acc).
  * conv3x3_c64_kernel<1, true> and the flat 64-wide data-gradient tiles with BatchNorm sums (F32ST) stage fp32: r = 1.
  * the ReLU mask multiplies by 0 or 1 and repacks an already representable value: no rounding.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24
U_BF16 = 2.0 ** -8


def bf16_round(a):
    """float32 numpy -> nearest bf16, as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _pair(fn, a, w):
    """fn on (a, w) and on (|a|, |w|), float64 numpy out."""
    a, w = _t64(a), _t64(w)
    return fn(a, w).numpy(), fn(a.abs(), w.abs()).numpy()


def conv_fwd(x, w, stride, pad):
    """y = conv2d(x [N,C,H,W], w [K,C,R,S])."""
    return _pair(lambda a, b: F.conv2d(a, b, stride=stride, padding=pad), x, w)


def _dgrad(dy, w, hw, stride, pad):
    H, W = hw
    R, S = w.shape[2], w.shape[3]
    P, Q = dy.shape[2], dy.shape[3]
    oph, opw = H - ((P - 1) * stride - 2 * pad + R), W - ((Q - 1) * stride - 2 * pad + S)
    assert 0 <= oph < stride and 0 <= opw < stride, (hw, dy.shape)
    return _pair(lambda a, b: F.conv_transpose2d(a, b, stride=stride, padding=pad, output_padding=(oph, opw)), dy, w)


def conv_dgrad_s1(dy, w, hw, pad):
    """dx [N,C,H,W] of a stride-1 convolution from dy [N,K,H,W] and w [K,C,R,S]."""
    return _dgrad(dy, w, hw, 1, pad)


def conv_dgrad_s2(dy, w, hw, pad):
    """dx of a stride-2 convolution; an odd H or W leaves input rows / columns no output pixel's last tap reaches."""
    return _dgrad(dy, w, hw, 2, pad)


def conv_dgrad_ds(dy, w, dy_ds, w_ds, hw):
    """The downsample pair: the 3x3 stride-2 pad-1 gradient plus the 1x1 stride-2 gradient, summed (mag too)."""
    r1, m1 = _dgrad(dy, w, hw, 2, 1)
    r2, m2 = _dgrad(dy_ds, w_ds, hw, 2, 0)
    return r1 + r2, m1 + m2


def stem_fwd(x5, w):
    """The 7x7 stride-2 pad-3 stem on x5 [B,Cin,T,H,W]: frames become images, [B*T,64,P,Q]."""
    B, Cin, T, H, W = x5.shape
    x4 = np.ascontiguousarray(np.transpose(x5, (0, 2, 1, 3, 4))).reshape(B * T, Cin, H, W)
    return conv_fwd(x4, w, 2, 3)


def bound(ref64, mag, n, u_out, r=1, extras=()):
    """The per-element bound of the module docstring.  extras: arrays broadcastable to ref64, each added once."""
    assert r in (1, 2)
    ext_abs = sum((np.abs(np.asarray(e, np.float64)) for e in extras), np.zeros((), np.float64))
    ext_sum = sum((np.asarray(e, np.float64) for e in extras), np.zeros((), np.float64))
    acc = 2.0 * (n + 1) * EPS32 * mag + 2.0 * EPS32 * ext_abs
    b = acc + u_out * (np.abs(ref64) + acc)
    if r == 2:
        b = b + u_out * (np.abs(ref64 - ext_sum) + acc)
    return b


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def check(got, ref64, bnd, *, zero_where=None, layout="nchw"):
    """|got - ref64| <= bnd at EVERY element (a NaN fails), got == 0 exactly where zero_where is set.  Returns the worst
    err / bound; raises AssertionError with the count and the ten worst offenders as (n, c, h, w, got, ref, err/bound), their
    GEMM row (n*H + h)*W + w, that row modulo 64 / 128 / 192 and whether the pixel lies on an image border."""
    assert layout in ("nchw", "nhwc")
    got = np.asarray(got, np.float64)
    if layout == "nhwc":
        got, ref64, bnd = (np.transpose(a, (0, 3, 1, 2)) for a in (got, ref64, np.broadcast_to(bnd, ref64.shape)))
        zero_where = None if zero_where is None else np.transpose(zero_where, (0, 3, 1, 2))
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    bnd = np.broadcast_to(bnd, ref64.shape)
    err = np.abs(got - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bnd)
    ratio = np.where(np.isfinite(got), ratio, np.inf)  # NaN / Inf in the output: never inside a bound
    bad = ~(ratio <= 1.0)
    if zero_where is not None:
        nz = zero_where & (got != 0)
        ratio = np.where(nz, np.inf, ratio)
        bad |= nz
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    if bad.any():
        N, C, H, W = ref64.shape
        idx = np.argwhere(bad)
        order = np.argsort(-np.nan_to_num(ratio[bad], nan=np.inf, posinf=np.finfo(np.float64).max))[:10]
        lines = []
        for n, c, h, w in idx[order]:
            row = (n * H + h) * W + w
            border = h in (0, H - 1) or w in (0, W - 1)
            lines.append(f"  (n={n}, c={c}, h={h}, w={w}) got={got[n, c, h, w]:.6g} ref={ref64[n, c, h, w]:.6g} "
                         f"err/bound={ratio[n, c, h, w]:.3g}  row={row} %64={row % 64} %128={row % 128} %192={row % 192} "
                         f"border={'yes' if border else 'no'}")
        raise AssertionError(f"{int(bad.sum())} of {bad.size} elements outside the bound (worst err/bound {worst:.3g}); the worst:\n"
                             + "\n".join(lines))
    return worst


BAND = 4096


def guarded(shape, dtype, poison, device="cuda:0", fill=None):
    """A tensor view of `shape` / `dtype` inside ONE buffer, with a 4 KiB guard band directly before and directly after it; the view
    starts 4096-byte aligned.  poison "nan": an input -- the bands are NaN (all-ones bytes).  poison "pattern": an output -- the bands
    hold a fixed byte pattern, the tensor itself NaN, or `fill` (the addend of an in-place launch).  Returns (view, check_bands);
    check_bands() asserts that both bands are byte-identical to what they were."""
    assert poison in ("nan", "pattern")
    esz = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape))
    buf = torch.empty(2 * BAND + n * esz + BAND, dtype=torch.uint8, device=device)
    off = (-buf.data_ptr()) % BAND + BAND  # first aligned address that leaves a whole band before it
    lo, mid, hi = buf[off - BAND:off], buf[off:off + n * esz], buf[off + n * esz:off + n * esz + BAND]
    if poison == "nan":
        lo.fill_(0xFF), hi.fill_(0xFF)
    else:
        pat = (torch.arange(BAND, dtype=torch.int32) * 37 + 11).remainder(251).to(torch.uint8).to(device)
        lo.copy_(pat), hi.copy_(pat.flip(0))
    mid.fill_(0xFF)
    view = mid.view(dtype).view(*shape)
    assert view.data_ptr() % BAND == 0
    if fill is not None:
        view.copy_(fill)
    keep_lo, keep_hi = lo.clone(), hi.clone()

    def check_bands(what=""):
        for name, now, was in (("before", lo, keep_lo), ("after", hi, keep_hi)):
            diff = (now != was).nonzero().flatten()
            assert diff.numel() == 0, (f"guard band {name} the tensor {what}: {diff.numel()} bytes changed, first at band offset "
                                       f"{int(diff[0])}")

    check_bands.buffer = buf  # (keeps the allocation alive with the closure; tests poke it)
    check_bands.bands = (lo, hi)
    return view, check_bands
