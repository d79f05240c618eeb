"""CPU-only checks of the AdamW / Adagrad updates behind DGLTrainer(optimizer="Adam" | "AdaGrad") (main_dgl.py --optimizer,
:248-259): the C ABI exports both, the float64 restatement the GPU op test measures against is torch.optim's arithmetic, and
the golden fixtures of the reference's Adam / AdaGrad steps were made with the script's hyperparameters."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optim_ref as ref  # noqa: E402
from gdl import _lib as L  # noqa: E402

NEW = ("gdl_optim_adamw_step", "gdl_optim_adagrad_step")


def test_abi_has_both_updates():
    src = open(os.path.join(ROOT, "include", "gdl_hip.h")).read()
    lib = ctypes.CDLL(L.SO_PATH)  # loads without a GPU
    for name in NEW:
        assert f"GDL_API int {name}(" in src, name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    # the step counter and the hyperparameters are 64-bit: int64 step, double lr / betas / eps / weight decay
    assert L.SIGNATURES["gdl_optim_adamw_step"] == ("i", "pppppp" + "f" + "ddddd" + "l" + "p")
    assert L.SIGNATURES["gdl_optim_adagrad_step"] == ("i", "ppppp" + "f" + "ddd" + "l" + "p")


def test_trainer_rejects_unknown_optimizer_before_allocating():
    from gdl.trainer import DEFAULT_WEIGHT_DECAY, OPTIMIZERS, DGLTrainer

    assert OPTIMIZERS == ("sgd", "Adam", "AdaGrad")  # main_dgl.py's own strings
    assert DEFAULT_WEIGHT_DECAY == {"sgd": 1e-4, "Adam": 1e-2, "AdaGrad": 0.0}
    for bad in ("adam", "AdamW", "adagrad", "SGD", None):
        with pytest.raises(ValueError):
            DGLTrainer(None, lr=1e-3, optimizer=bad)  # (a model would be touched only after the check)


SIZES = [7, 33, 130, 1]


def _torch_run(kind, steps, scale, lr=2e-3):
    """torch.optim on float64 CPU tensors (foreach=False, the reference's arguments) with clip_grad_norm_(.., 40) before each
    step; and the restatement over the flat arena on the same gradients."""
    rng = np.random.default_rng(11)
    p0 = [rng.standard_normal(n) for n in SIZES]
    params = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p0]
    opt = (torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.999), foreach=False) if kind == "Adam"
           else torch.optim.Adagrad(params, lr=lr, foreach=False))
    p = np.concatenate(p0)
    s1, s2 = np.zeros_like(p), np.zeros_like(p)
    coefs = []
    for t in range(1, steps + 1):
        g = [scale * rng.standard_normal(n) for n in SIZES]
        for x, gg in zip(params, g):
            x.grad = torch.tensor(gg, dtype=torch.float64)
        torch.nn.utils.clip_grad_norm_(params, max_norm=40, norm_type=2)
        opt.step()
        gc, _, coef = ref.clip(np.concatenate(g))
        coefs.append(coef)
        if kind == "Adam":
            p, s1, s2 = ref.adamw(p, gc, s1, s2, lr, t)
        else:
            p, s1 = ref.adagrad(p, gc, s1, lr)
    keys = ("exp_avg", "exp_avg_sq") if kind == "Adam" else ("sum",)
    want_p = np.concatenate([x.detach().numpy() for x in params])
    want_s = [np.concatenate([opt.state[x][k].numpy() for x in params]) for k in keys]
    return (p, [s1, s2][:len(keys)]), (want_p, want_s), coefs


@pytest.mark.parametrize("kind", ["Adam", "AdaGrad"])
@pytest.mark.parametrize("scale", [0.1, 30.0])  # the clip inactive / active
def test_restatement_matches_torch_optim(kind, scale):
    (p, states), (want_p, want_s), coefs = _torch_run(kind, 5, scale)
    assert (max(coefs) < 1.0) if scale > 1 else all(c == 1.0 for c in coefs)
    np.testing.assert_allclose(p, want_p, rtol=1e-12, atol=1e-14)
    for got, want in zip(states, want_s):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("name,kind", [("dgl_adamw_tiny_b4", "Adam"), ("dgl_adagrad_tiny_b4", "AdaGrad"),
                                       ("dgl_swin_adamw_tiny_b4", "Adam")])
def test_optimizer_goldens_record_the_script_hyperparameters(golden_dir, name, kind):
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    cfg = json.loads(str(g["config"]))
    assert cfg["optimizer"] == kind and cfg["steps"] == 3 and cfg["mode"] == "dgl" and cfg["max_norm"] == 40.0
    a = cfg["optimizer_args"]
    if kind == "Adam":  # optim.AdamW(model.parameters(), lr=args.learning_rate, betas=(0.9, 0.999))   (main_dgl.py:255)
        assert cfg["optimizer_torch"] == "AdamW"
        assert a["betas"] == [0.9, 0.999] and a["eps"] == ref.ADAMW["eps"] and a["weight_decay"] == ref.ADAMW["weight_decay"]
        assert a["amsgrad"] is False and a["maximize"] is False
        assert list(g["state_keys"]) == ["exp_avg", "exp_avg_sq"]
    else:  # optim.Adagrad(model.parameters(), lr=args.learning_rate)                                   (main_dgl.py:253)
        assert cfg["optimizer_torch"] == "Adagrad"
        assert a["eps"] == ref.ADAGRAD["eps"] and a["weight_decay"] == 0 and a["lr_decay"] == 0
        assert a["initial_accumulator_value"] == 0 and a["maximize"] is False
        assert list(g["state_keys"]) == ["sum"]
    assert a["lr"] == cfg["lr"]
    for st in range(3):
        assert g[f"s{st}.param_sums"].shape == (len(g[f"s{st}.grad_names"]), 2)
        assert g[f"s{st}.state_sums"].shape[1:] == (len(g["state_keys"]), 2)
    assert os.path.getsize(os.path.join(golden_dir, name + ".npz")) < 1 << 20
