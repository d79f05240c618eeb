"""float64 NumPy restatement of the concat / sum DGL head without its .detach(), the three cross-entropies and the backward
under the two ablation flags (the C ABI's `out_reaches_xy` / `fused_reaches` and `uni_in_dw`):

  out_a = x Wa^T + ba,  out_v = y Wv^T + bv,  out = x Wa^T + y Wv^T + bias
      concat: Wa = W[:, :512], Wv = W[:, 512:], ba = bv = bias = fc_out.bias
      sum:    Wa = fc_x.weight, Wv = fc_y.weight, their biases, bias = ba + bv
  loss_* = mean CE;  g_f = dCE(out),  g_a = alpha dCE(out_a),  g_v = alpha dCE(out_v)
  dx = (g_a + reach g_f) Wa,  dy = (g_v + reach g_f) Wv
  dWa = (g_f + uni g_a)^T x,  dWv = (g_f + uni g_v)^T y;  concat: db = sum_b (g_f + uni (g_a + g_v)); sum: dba, dbv likewise each

Used by the tests at shapes that have no fixture."""
import numpy as np


def split_params(kind, params):
    """(Wa, Wv, ba, bv, sum_bias) in float64 from the head's tensors: concat (W [n,1024], b) or sum (Wx, bx, Wy, by)."""
    P = [np.asarray(p, dtype=np.float64) for p in params]
    if kind == "concat":
        W, b = P
        return W[:, :512], W[:, 512:], b, b, False
    Wx, bx, Wy, by = P
    return Wx, Wy, bx, by, True


def ce(logits, labels):
    """(mean loss, d loss / d logits) of nn.CrossEntropyLoss on float64 logits"""
    B = logits.shape[0]
    z = logits - logits.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z).sum(axis=1, keepdims=True))
    logp = z - lse
    onehot = np.zeros_like(logits)
    onehot[np.arange(B), labels] = 1.0
    return float(-(logp[np.arange(B), labels]).mean()), (np.exp(logp) - onehot) / B


def head(kind, params, x, y, labels, alpha, reach, uni):
    """Everything the head computes in one training step; `reach`, `uni`: the two flags (0 / 1).  Returns a dict: out, out_a, out_v,
    loss_f, loss_a, loss_v, g_f, g_a, g_v, dx, dy and `grads` (the parameter gradients in the order of `params`)."""
    Wa, Wv, ba, bv, sum_bias = split_params(kind, params)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    labels = np.asarray(labels)
    pa, pv = x @ Wa.T, y @ Wv.T
    out_a, out_v = pa + ba, pv + bv
    out = pa + pv + (ba + bv if sum_bias else ba)
    loss_f, g_f = ce(out, labels)
    loss_a, g_a = ce(out_a, labels)
    loss_v, g_v = ce(out_v, labels)
    g_a, g_v = alpha * g_a, alpha * g_v
    dx = (g_a + reach * g_f) @ Wa
    dy = (g_v + reach * g_f) @ Wv
    dWa, dWv = (g_f + uni * g_a).T @ x, (g_f + uni * g_v).T @ y
    if sum_bias:
        grads = [dWa, (g_f + uni * g_a).sum(0), dWv, (g_f + uni * g_v).sum(0)]
    else:
        grads = [np.concatenate([dWa, dWv], axis=1), (g_f + uni * (g_a + g_v)).sum(0)]
    return dict(out=out, out_a=out_a, out_v=out_v, loss_f=loss_f, loss_a=loss_a, loss_v=loss_v, g_f=g_f, g_a=g_a, g_v=g_v,
                dx=dx, dy=dy, grads=grads)
