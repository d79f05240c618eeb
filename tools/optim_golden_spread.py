#!/usr/bin/env python3
"""How far two runs of the Adam / AdaGrad golden fixtures (tests/golden/dgl_{adamw,adagrad,swin_adamw}_tiny_b4.npz) lie from the
float32 goldens, step by step: what tests/test_optimizers_gpu.py's BOUNDS were set from.

    python tools/optim_golden_spread.py --side mi355x --base profiles/optimizers_golden_spread.json --out FILE
        DGLTrainer(optimizer=...) in f32 on the GPU (tests/test_optimizers_gpu.py::run_golden)
    python tests/golden/make_golden_optim.py --float64 DIR     (where the reference is importable)
    python tools/optim_golden_spread.py --side reference_f64 --against DIR --out FILE
        the reference's own step, model and inputs in float64

--base: an earlier output whose other sides are kept.  The output: {side: {fixture: [per step {metric: value}]}}, the
metrics named like BOUNDS' keys:
  logit  max |got - golden| over the three logit sets        loss   max |got - golden| over loss_f, loss_a, loss_v
  norm   |got - golden| / golden of the total gradient norm  gsum   the same, worst of audio_grad_sum / visual_grad_sum
  gnorm  the same, worst per-tensor gradient norm            psum   the same, worst per-tensor sum|p| after the update
  state  the same, worst per-tensor sum|state| (each state tensor; entries below 1e-6 of their column's largest are left
         out -- the test's atol covers them)
  buf    max |got - golden| over the BatchNorm buffers
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-gdl_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

FIXTURES = ["dgl_adamw_tiny_b4", "dgl_adagrad_tiny_b4", "dgl_swin_adamw_tiny_b4"]


def _rel(a, b):
    return float(abs(a - b) / abs(b))


def metrics(g, st, got):
    """`got`: one step of the compared run -- out / out_a / out_v, the three losses, total_norm, the two grad sums,
    grad_norm {name: value}, psum / ssum aligned with the golden's tensor names, bufs {name: array}."""
    pre = f"s{st}."
    names = [str(n) for n in g[pre + "grad_names"]]
    gn, isnone = g[pre + "grad_norm"], g[pre + "grad_is_none"]
    ws = g[pre + "state_sums"][:, :, 1]
    keep = ws > 1e-6 * ws.max(axis=0, keepdims=True)
    ps = g[pre + "param_sums"][:, 1]
    return {"logit": float(max(np.abs(np.asarray(got[k]) - g[pre + k]).max() for k in ("out", "out_a", "out_v"))),
            "loss": float(max(abs(float(got[k]) - float(g[pre + k])) for k in ("loss_f", "loss_a", "loss_v"))),
            "norm": _rel(got["total_norm"], float(g[pre + "total_norm"])),
            "gsum": max(_rel(got[k], float(g[pre + k])) for k in ("audio_grad_sum", "visual_grad_sum")),
            "gnorm": max(_rel(got["grad_norm"][n], gn[i]) for i, n in enumerate(names) if not isnone[i]),
            "psum": float((np.abs(got["psum"] - ps) / ps).max()),
            "state": float((np.abs(got["ssum"] - ws) / np.where(keep, ws, 1.0))[keep].max()),
            "buf": float(max(np.abs(got["bufs"][k] - g[pre + "buf." + k]).max() for k in got["bufs"]))}


def side_mi355x(name):
    import test_optimizers_gpu as T

    g, cfg, out = T.run_golden(name)
    res = []
    for st, (r, psum, ssum, bufs) in enumerate(out):
        res.append(metrics(g, st, {**r, "psum": psum, "ssum": ssum, "bufs": bufs}))
    return res


def side_fixture(name, d):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    h = np.load(os.path.join(d, name + ".npz"))
    res = []
    for st in range(json.loads(str(g["config"]))["steps"]):
        pre = f"s{st}."
        names = [str(n) for n in h[pre + "grad_names"]]
        got = {k: h[pre + k] for k in ("out", "out_a", "out_v", "loss_f", "loss_a", "loss_v", "total_norm", "audio_grad_sum",
                                       "visual_grad_sum")}
        got.update(grad_norm=dict(zip(names, h[pre + "grad_norm"].tolist())), psum=h[pre + "param_sums"][:, 1],
                   ssum=h[pre + "state_sums"][:, :, 1],
                   bufs={k[len(pre + "buf."):]: h[k].astype(np.float64) for k in h.files if k.startswith(pre + "buf.")})
        res.append(metrics(g, st, got))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", required=True, choices=["mi355x", "reference_f64"])
    ap.add_argument("--against", help="directory of make_golden_optim.py --float64 (reference_f64)")
    ap.add_argument("--base", help="earlier output to extend")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    out = json.load(open(a.base)) if a.base and os.path.exists(a.base) else {}
    if a.side == "mi355x":
        out[a.side] = {n: side_mi355x(n) for n in FIXTURES}
    else:
        out[a.side] = {n: side_fixture(n, a.against) for n in FIXTURES}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    for n in FIXTURES:
        for st, m in enumerate(out[a.side][n]):
            print(a.side, n, st, " ".join(f"{k} {v:.3g}" for k, v in m.items()))


if __name__ == "__main__":
    main()
