"""float64 NumPy restatement of the linear probe's fused fit (csrc/linprobe.hip, include/gdl_hip.h "linear probe"): main.py's
unimodal step with the encoder removed, on the bank rows an order table names --
    out = f W^T + b;  loss = mean CE(out, y);  dW = dlogits^T f, db = sum_b dlogits,  dlogits = (softmax(out) - onehot) / B
    clip_grad_norm_({dW, db}, max_norm):  coef = min(1, max_norm / (norm + 1e-6))
    SGD:  d = coef g + wd p;  m = mu m + d;  p -= lr m        (momentum starts at zero: the first step's m is d, as torch's)
A label outside [0, n) gives no one-hot term and a NaN loss term (gdl_softmax_ce's rule); the other samples are unaffected.
Shared by tests/test_probe_cpu.py (against torch's float32 trajectories) and tests/test_probe_gpu.py (the kernels against it).
"""
import numpy as np


def step(W, b, mW, mb, f, y, lr, mu, wd, max_norm):
    """One step in place on float64 W [n, 512], b [n], mW, mb; f [B, 512], y [B].  Returns (mean loss, pre-clip norm)."""
    B, n = f.shape[0], W.shape[0]
    out = f @ W.T + b
    mx = out.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(out - mx).sum(axis=1))
    ok = (y >= 0) & (y < n)
    yc = np.where(ok, y, 0)
    term = np.where(ok, lse - out[np.arange(B), yc], np.nan)
    onehot = np.zeros((B, n))
    onehot[np.arange(B)[ok], yc[ok]] = 1.0
    dl = (np.exp(out - lse[:, None]) - onehot) / B
    dW, db = dl.T @ f, dl.sum(axis=0)
    norm = float(np.sqrt((dW * dW).sum() + (db * db).sum()))
    coef = min(1.0, max_norm / (norm + 1e-6))
    for p, g, m in ((W, dW, mW), (b, db, mb)):
        m *= mu
        m += coef * g + wd * p
        p -= lr * m
    return float(term.sum() / B), norm


def fit(bank, labels, order, W, b, mW=None, mb=None, lr=1e-3, mu=0.9, wd=1e-4, max_norm=40.0):
    """order [epochs, steps, B]; lr a float or one per epoch.  Returns a list per epoch of dicts W, b, mW, mb (copies), loss (the
    mean of the steps' mean losses) and norms (the steps' pre-clip gradient norms).  The inputs are not modified."""
    bank = np.asarray(bank, dtype=np.float64)
    labels = np.asarray(labels)
    W, b = np.array(W, dtype=np.float64), np.array(b, dtype=np.float64)
    mW = np.zeros_like(W) if mW is None else np.array(mW, dtype=np.float64)
    mb = np.zeros_like(b) if mb is None else np.array(mb, dtype=np.float64)
    order = np.asarray(order)
    lrs = [float(lr)] * order.shape[0] if np.ndim(lr) == 0 else [float(v) for v in lr]
    traj = []
    for e in range(order.shape[0]):
        losses, norms = [], []
        for idx in order[e]:
            l, nm = step(W, b, mW, mb, bank[idx], labels[idx], lrs[e], mu, wd, max_norm)
            losses.append(l)
            norms.append(nm)
        traj.append(dict(W=W.copy(), b=b.copy(), mW=mW.copy(), mb=mb.copy(), loss=float(np.sum(losses) / max(len(losses), 1)),
                         norms=np.array(norms)))
    return traj


def torch_fit(bank, labels, order, W, b, lr=1e-3, mu=0.9, wd=1e-4, max_norm=40.0):
    """The same fit by torch on the CPU in float32 -- nn.Linear + CrossEntropyLoss + clip_grad_norm_ + optim.SGD, what the
    scripts' step is made of -- in fit()'s return format (loss: the float64 sum of the steps' float32 `.item()`s, as the
    scripts add them).  Labels must be in range."""
    import torch

    order = np.asarray(order)
    lin = torch.nn.Linear(W.shape[1], W.shape[0])
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(np.asarray(W, dtype=np.float32)))
        lin.bias.copy_(torch.from_numpy(np.asarray(b, dtype=np.float32)))
    lrs = [float(lr)] * order.shape[0] if np.ndim(lr) == 0 else [float(v) for v in lr]
    opt = torch.optim.SGD(lin.parameters(), lr=lrs[0], momentum=mu, weight_decay=wd)
    crit = torch.nn.CrossEntropyLoss()
    fb = torch.from_numpy(np.asarray(bank, dtype=np.float32))
    yb = torch.from_numpy(np.asarray(labels, dtype=np.int64))
    traj = []
    for e in range(order.shape[0]):
        for g in opt.param_groups:
            g["lr"] = lrs[e]
        losses, norms = [], []
        for idx in order[e]:
            idx = torch.from_numpy(np.asarray(idx, dtype=np.int64))
            opt.zero_grad()
            loss = crit(lin(fb[idx]), yb[idx])
            loss.backward()
            norms.append(float(torch.nn.utils.clip_grad_norm_(lin.parameters(), max_norm)))
            opt.step()
            losses.append(loss.item())
        st = opt.state
        traj.append(dict(W=lin.weight.detach().numpy().copy(), b=lin.bias.detach().numpy().copy(),
                         mW=st[lin.weight]["momentum_buffer"].numpy().copy(), mb=st[lin.bias]["momentum_buffer"].numpy().copy(),
                         loss=float(np.sum(losses) / max(len(losses), 1)), norms=np.array(norms)))
    return traj


# the synthetic cases of the kernel tests: (N, B, n) and what each exercises
CASES = [
    (5, 1, 1),         # smallest case
    (12, 4, 6),        # the golden's shape
    (70, 3, 33),       # B does not divide N; n crosses the 32-class stride of head_body.h's wave loop
    (300, 64, 34),     # mid-size batch and class count
    (520, 257, 309),   # crosses the 256-way loss-sum fold
    (40, 8, 512),      # the class limit
]
CLIP_NORM = 0.02  # a max_norm every step of every case exceeds (asserted where it is used)
HYPER = dict(lr=1e-2, mu=0.9, wd=1e-4)


def synthetic_case(N, B, n, epochs=2):
    """A seeded bank (non-negative, as pooled ReLU features are), labels, Xavier-scaled W, a small bias and an order table of
    `epochs` permutations with the ragged tail dropped."""
    r = np.random.default_rng([20251, N, B, n])
    bank = np.abs(r.standard_normal((N, 512))).astype(np.float32)
    labels = r.integers(0, n, size=N).astype(np.int64)
    W = (r.standard_normal((n, 512)) * np.sqrt(2.0 / (512 + n))).astype(np.float32)
    b = (0.1 * r.standard_normal(n)).astype(np.float32)
    steps = N // B
    order = np.stack([r.permutation(N)[:steps * B].reshape(steps, B) for _ in range(epochs)]).astype(np.int32)
    return bank, labels, W, b, order


# Largest deviation() / loss_deviation() of torch_fit (CPU, float32) from fit (float64) over CASES x {max_norm 40, CLIP_NORM},
# 2 epochs, HYPER -- measured with tools/bench_probe.py --spread (docs/parity_log.md "Linear probe"): the float32 noise of this
# fit.  The kernels are another float32 fit that differs from torch's only in summation order: they are held to 4 x these.
TORCH32_DEV = dict(W=3.34e-7, b=2.31e-7, mW=1.69e-5, mb=1.52e-5, loss=8.93e-8)
BOUND = {k: 4.0 * v for k, v in TORCH32_DEV.items()}


# The same measurement on the fixtures tests/golden/probe_*_tiny.npz (their torch float32 trajectories against fit() from
# their start: 2 fixtures x 2 runs x 3 epochs, lr 1e-2; `tools/bench_probe.py --spread` prints it too).  Their bias starts at
# zero and stays below 0.015 while each step moves it by sums of order 1e-2: its float32 noise relative to max |b| is three
# times the synthetic cases', so the fixtures carry figures of their own.  A float32 fit is held to 4 x these against the
# restatement, and to 5 x these against the fixture itself (the fixture's own 1 x plus the 4 x).
GOLDEN32_DEV = dict(W=1.62e-7, b=7.22e-7, mW=3.11e-7, mb=3.74e-7, loss=7.75e-8)


def loss_deviation(got, want):
    """|got - want| / max(1, |want|): relative for the usual losses above 1, absolute below (n = 1 has loss 0)."""
    return abs(float(got) - float(want)) / max(1.0, abs(float(want)))


def deviation(got, want):
    """The kernel tests' measure: max |got - want| / max(1e-30, max |want|) of one array -- the error relative to the array's
    largest entry (entries near zero are not asked for more digits than the sums that made them carry)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(1e-30, np.abs(want).max()))
