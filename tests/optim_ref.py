"""float64 NumPy restatement of the clip and of the two optimizers main_dgl.py builds besides SGD (:252-256), over a flat
arena: the yardstick of tests/test_optimizers_gpu.py's op-level test, itself pinned against torch.optim by
tests/test_optimizers_cpu.py.  No GPU, no reference import."""
import numpy as np

# main_dgl.py:252-256: torch.optim.AdamW(lr, betas=(0.9, 0.999)) and torch.optim.Adagrad(lr), torch's defaults otherwise
ADAMW = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
ADAGRAD = dict(eps=1e-10, weight_decay=0.0, lr_decay=0.0, initial_accumulator_value=0.0)


def clip(g, max_norm=40.0, grad_scale=1.0):
    """clip_grad_norm_(.., max_norm, 2) of the gradient g * grad_scale: (clipped gradient, total norm, clip coefficient)."""
    g = np.asarray(g, np.float64) * grad_scale
    total = float(np.sqrt(np.sum(g * g)))
    coef = min(1.0, max_norm / (total + 1e-6))
    return g * coef, total, coef


def adamw(p, g, m, v, lr, step, betas=ADAMW["betas"], eps=ADAMW["eps"], weight_decay=ADAMW["weight_decay"]):
    """torch's _single_tensor_adam with decoupled weight decay (AdamW), step counted from 1; returns new (p, m, v)."""
    b1, b2 = betas
    p = p * (1.0 - lr * weight_decay)
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** step)
    bc2_sqrt = np.sqrt(1.0 - b2 ** step)
    return p - step_size * m / (np.sqrt(v) / bc2_sqrt + eps), m, v


def adagrad(p, g, s, lr, eps=ADAGRAD["eps"], weight_decay=ADAGRAD["weight_decay"]):
    """torch's _single_tensor_adagrad with lr_decay 0; returns new (p, s)."""
    d = g + weight_decay * p
    s = s + d * d
    return p - lr * d / (np.sqrt(s) + eps), s
