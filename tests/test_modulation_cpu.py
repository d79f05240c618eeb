"""CPU-only checks of what the GPU tests of OGM / OGM-GE gradient modulation are measured against (tests/modulation_ref.py):
the Philox4x32-10 known-answer vectors, the moments of the reference normals, the coefficient rule against a torch restatement of
main.py:286-306 -- and the refusal that needs no model."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import modulation_ref as mref  # noqa: E402

KAT = [  # counter, key -> output (Random123's known-answer vectors of philox4x32-10)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = mref.philox4x32_10(ctr, key)
    assert tuple(int(w) for w in got) == want


def test_philox_vectorised_equals_scalar():
    """the array form the other tests use gives each element what the scalar call gives"""
    c0 = np.array([0, 0xffffffff, 0x243f6a88], dtype=np.uint64)
    got = mref.philox4x32_10((c0, 7, 3, 0), (11, 13))
    for i, c in enumerate(c0.tolist()):
        one = mref.philox4x32_10((c, 7, 3, 0), (11, 13))
        assert [int(w[i]) for w in got] == [int(w) for w in one]


def test_uniform_is_open_interval():
    u = mref.uniform(np.array([0, 0xff, 0x100, 0xffffffff], dtype=np.uint32))
    assert u[0] == u[1] == 2.0 ** -25 and u[2] == 1.5 * 2.0 ** -24 and u[3] == 1.0 - 2.0 ** -25


def test_reference_normals_moments():
    """10^6 reference normals: mean, variance and excess kurtosis within 5 standard errors (1/sqrt N, sqrt(2/N), sqrt(24/N))."""
    N = 10 ** 6
    z = mref.normals(np.arange(N, dtype=np.int64), seed=0x1234567887654321 & (2 ** 63 - 1), step=5)
    assert z.shape == (N,) and np.isfinite(z).all()
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2 - 3.0
    print("moments", mean, var, kurt)
    assert abs(mean) < 5 / np.sqrt(N)
    assert abs(var - 1) < 5 * np.sqrt(2 / N)
    assert abs(kurt) < 5 * np.sqrt(24 / N)
    # lanes of one counter are distinct draws; another step or seed is another stream
    assert len(np.unique(z[:4])) == 4
    assert not np.array_equal(z[:64], mref.normals(np.arange(64), seed=0x1234567887654321 & (2 ** 63 - 1), step=6))
    assert not np.array_equal(z[:64], mref.normals(np.arange(64), seed=1, step=5))


def _torch_coefficients(out_a, out_v, label, alpha):
    """main.py:286-306 as written there (float32 torch)"""
    softmax, tanh, relu = torch.nn.Softmax(dim=1), torch.nn.Tanh(), torch.nn.ReLU(inplace=True)
    score_v = sum([softmax(out_v)[i][label[i]] for i in range(out_v.size(0))])
    score_a = sum([softmax(out_a)[i][label[i]] for i in range(out_a.size(0))])
    ratio_v = score_v / score_a
    ratio_a = 1 / ratio_v
    if ratio_v > 1:
        coeff_v = 1 - tanh(alpha * relu(ratio_v))
        coeff_a = 1
    else:
        coeff_a = 1 - tanh(alpha * relu(ratio_a))
        coeff_v = 1
    return float(score_a), float(score_v), float(ratio_v), float(coeff_a), float(coeff_v)


def test_coefficients_against_torch():
    """Scores and coefficients on random logits agree with the torch restatement to float32's precision, on both branches."""
    seen = set()
    for case in range(12):
        r = np.random.default_rng([77, case])
        B, n = 7, 6
        label = r.integers(0, n, B)
        out_a = r.standard_normal((B, n)).astype(np.float32) * (2.0 if case % 2 else 0.5)
        out_v = r.standard_normal((B, n)).astype(np.float32) * (0.5 if case % 2 else 2.0)
        out_a[np.arange(B), label] += 1.0 if case % 3 else -1.0
        sa, sv = mref.label_probs(out_a, label).sum(), mref.label_probs(out_v, label).sum()
        rv, ca, cv = mref.coefficients(sa, sv, 0.8)
        want = _torch_coefficients(torch.from_numpy(out_a), torch.from_numpy(out_v), torch.from_numpy(label), 0.8)
        np.testing.assert_allclose([sa, sv, rv], want[:3], rtol=1e-5)
        np.testing.assert_allclose([ca, cv], want[3:], rtol=1e-4, atol=1e-6)  # (float32's 1 - tanh cancels)
        assert (ca == 1.0) == (rv > 1) and (cv == 1.0) == (not rv > 1)
        seen.add(rv > 1)
    assert seen == {True, False}


def test_ratio_one_takes_the_audio_branch():
    rv, ca, cv = mref.coefficients(1.25, 1.25, 0.8)
    assert rv == 1.0 and cv == 1.0 and ca == pytest.approx(1.0 - np.tanh(0.8))


def test_modulate_reference():
    """the arena restatement: unmarked segments are g k, OGM scales by the modality's coefficient, GE adds sigma z of the
    clipped tensor's unbiased standard deviation"""
    r = np.random.default_rng(3)
    offs = [0, 5, 11, 30]
    g = r.standard_normal(30).astype(np.float32)
    out, sig = mref.modulate(g, offs, [0, 1, 2], 0.5, 0.25, 1.0, False)
    gk = (g * np.float32(0.5)).astype(np.float64)
    np.testing.assert_array_equal(out[:5], gk[:5])
    np.testing.assert_array_equal(out[5:11], gk[5:11] * 0.25)
    np.testing.assert_array_equal(out[11:], gk[11:])
    assert not sig.any()
    out2, sig = mref.modulate(g, offs, [0, 1, 2], 0.5, 0.25, 1.0, True, seed=9, step=2)
    assert sig[0] == 0 and sig[2] == pytest.approx(torch.from_numpy(gk[11:]).std().item() + 1e-8, rel=1e-12)
    np.testing.assert_allclose((out2 - out)[11:] / sig[2], mref.normals(np.arange(11, 30), 9, 2), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(out2[:5], out[:5])


def test_unknown_modulation_is_refused_before_the_model():
    """A wrong --modulation is a ValueError from a classmethod, raised before the model is touched (there is none here)."""
    from gdl.trainer import MODULATIONS, DGLTrainer

    assert MODULATIONS == ("Normal", "OGM", "OGM_GE")
    with pytest.raises(ValueError, match="modulation"):
        DGLTrainer(None, lr=1e-3, mode="joint", modulation="OGM-GE")
    with pytest.raises(ValueError, match="modulation"):
        DGLTrainer._check_modulation("ogm")
    for m in MODULATIONS:
        DGLTrainer._check_modulation(m)
