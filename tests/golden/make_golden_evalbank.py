"""Writes tests/golden/evalbank_small.npz: small float32 logit sets with labels, and scikit-learn's per-class
average_precision_score of the restatement's float32 probabilities (tests/evalbank_ref.py), recorded where scikit-learn is
installed so that neither the CPU nor the GPU tests need it.

    python tests/golden/make_golden_evalbank.py

Each case is a handful of distinct random rows, every one repeated three times under independent labels: repeated rows give
bit-equal probabilities on any evaluation (real ties, between positives and negatives too), and the generator asserts that
distinct rows' probabilities of a class lie at least 1e-4 apart relatively -- a thousand float32 roundings -- so that the
order of the scores, and with it the exact AP, is the same for the restatement's float64 softmax and the device's float32 one.
Every class has a positive (scikit-learn's 0.0 for an empty class is not the bank's NaN)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import evalbank_ref as er  # noqa: E402

CASES = {"a": (20, 5), "b": (11, 2), "c": (30, 9)}  # name -> (distinct rows, classes); N = 3 x rows


def make_case(name):
    rows, n = CASES[name]
    r = np.random.default_rng([2033, rows, n])
    lg = np.repeat((2.0 * r.standard_normal((rows, n))).astype(np.float32), 3, axis=0)
    lab = r.integers(0, n, 3 * rows).astype(np.int64)
    lab[:n] = np.arange(n)  # every class has a positive
    return lg, lab


def main():
    from sklearn.metrics import average_precision_score

    out = {}
    for name, (rows, n) in CASES.items():
        lg, lab = make_case(name)
        p64, _ = er.softmax_bound(lg)
        for c in range(n):
            v = np.unique(p64[:, c])
            assert v.size == rows and (np.diff(v) / v[1:]).min() > 1e-4, (name, c)
        p32 = p64.astype(np.float32)
        ap = np.array([average_precision_score((lab == c).astype(int), p32[:, c]) for c in range(n)])
        out[name + ".logits"], out[name + ".labels"], out[name + ".ap"] = lg, lab, ap
    np.savez(os.path.join(HERE, "evalbank_small.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
