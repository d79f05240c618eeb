"""CPU tests of the MMPareto arithmetic as tests/pareto_ref.py restates it: gamma is the minimiser it claims
to be, the integrated gradient does not conflict with either input where they agree, its norm is the plain sum's in both
branches, and the coefficients recorded in the step goldens are the restatement's for the goldens' recorded sums."""
import json
import os

import numpy as np
import pytest

import pareto_ref as pr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ["pareto_concat_tiny_b4", "pareto_sum_tiny_b4", "pareto_concat_a1_tiny_b4"]  # the last: alpha = 1.0, an interior gamma


def _pair(seed, n=257, mix=0.0, ratio=1.0):
    """two float32 vectors with cosine about `mix` and norm ratio about `ratio`"""
    rs = np.random.default_rng([7, seed])
    a = rs.standard_normal(n)
    b = rs.standard_normal(n)
    g_m = a.astype(np.float32)
    g_u = (ratio * (mix * a + np.sqrt(max(0.0, 1.0 - mix * mix)) * b)).astype(np.float32)
    return g_m, g_u


CASES = [(s, mix, ratio) for s, (mix, ratio) in enumerate([(0.3, 1.0), (0.6, 0.5), (0.1, 2.0), (0.9, 3.0), (0.9, 1.0 / 3.0), (0.5, 1.2),
                                                           (-0.4, 1.0), (-0.8, 0.7)])]


@pytest.mark.parametrize("seed,mix,ratio", CASES)
def test_gamma_minimises_the_segment(seed, mix, ratio):
    """gamma against a scan of the segment [g_u, g_m] in steps of 1e-4: no scanned point has a smaller norm (beyond rounding), and
    gamma lies within one step of the scan's arg-min.  In the sum branch (S_mu <= 0) nothing is minimised: gamma = 0.5, w = 1."""
    g_m, g_u = _pair(seed, mix=mix, ratio=ratio)
    c = pr.coefficients(*pr.sums(g_m, g_u))
    if c["branch"] == 0:
        assert mix < 0 and (c["gamma"], c["w_m"], c["w_u"], c["s"]) == (0.5, 1.0, 1.0, 1.0)
        return
    a, b = g_m.astype(np.float64), g_u.astype(np.float64)
    grid = np.arange(0, 10001) * 1e-4
    norms = np.array([np.sum((t * a + (1 - t) * b) ** 2) for t in grid])
    mine = np.sum((c["gamma"] * a + (1 - c["gamma"]) * b) ** 2)
    assert mine <= norms.min() * (1 + 1e-12)
    assert abs(grid[int(np.argmin(norms))] - c["gamma"]) <= 1e-4 + 1e-12
    assert c["w_m"] == 2 * c["gamma"] and c["w_u"] == 2 * (1 - c["gamma"])


@pytest.mark.parametrize("seed,mix,ratio", CASES)
def test_no_conflict_and_the_sums_norm(seed, mix, ratio):
    """Agreement branch: <g, g_m> >= 0 and <g, g_u> >= 0 (the min-norm point of two vectors with a positive dot product conflicts
    with neither), and s >= 1.  Both branches: ||g|| = ||g_m + g_u|| to 1e-12 relative, with the unrounded coefficients (the
    float32 rounding of c_m, c_u is the kernel's and is bounded in the GPU tests)."""
    g_m, g_u = _pair(seed, mix=mix, ratio=ratio)
    c = pr.coefficients(*pr.sums(g_m, g_u))
    a, b = g_m.astype(np.float64), g_u.astype(np.float64)
    g = c["s"] * (c["w_m"] * a + c["w_u"] * b)
    if c["branch"] == 1:
        assert np.dot(g, a) >= 0 and np.dot(g, b) >= 0
        assert c["s"] >= 1 - 1e-12
    want = np.linalg.norm(a + b)
    assert abs(np.linalg.norm(g) - want) <= 1e-12 * want
    g32, _ = pr.integrate(g_m, g_u)
    assert abs(np.linalg.norm(g32) - want) <= 4 * pr.U * want


def test_edge_cases():
    """D == 0 gives gamma 0.5; a zero vector, disjoint supports and a non-finite sum take the sum branch with s = 1 exactly;
    collinear vectors clamp and come out as the plain sum."""
    x = np.arange(1, 9, dtype=np.float32)
    c = pr.coefficients(*pr.sums(x, x))
    assert (c["branch"], c["gamma"], c["w_m"], c["w_u"], c["s"]) == (1, 0.5, 1.0, 1.0, 1.0)
    for g_m, g_u in ((x, 0 * x), (0 * x, 0 * x), (np.r_[x, 0 * x], np.r_[0 * x, x])):
        c = pr.coefficients(*pr.sums(g_m, g_u))
        assert (c["branch"], c["w_m"], c["w_u"], c["s"], c["c_m"], c["c_u"]) == (0, 1.0, 1.0, 1.0, 1.0, 1.0)
    bad = x.copy()
    bad[3] = np.nan
    g, c = pr.integrate(x, bad)
    assert c["branch"] == 0 and c["s"] == 1.0 and np.isnan(g[3]) and np.array_equal(np.delete(g, 3), np.delete(2.0 * x, 3))
    g, c = pr.integrate(3 * x, x)  # g_m = 3 g_u: gamma clamps to 0, 2 s g_u = 4 g_u = g_m + g_u
    assert c["gamma"] == 0.0 and c["branch"] == 1 and np.allclose(g, 4.0 * x, rtol=1e-6, atol=0)
    g, c = pr.integrate(x, 3 * x)  # g_u = 3 g_m: gamma clamps to 1
    assert c["gamma"] == 1.0 and c["branch"] == 1 and np.allclose(g, 4.0 * x, rtol=1e-6, atol=0)
    g, c = pr.integrate(x, x, scale=0.25)
    assert c["c_m"] == 0.25 and c["c_u"] == 0.25


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_coefficients_follow_from_the_recorded_sums(name):
    """Every (step, encoder) of the step goldens: the recorded gamma, w_m, w_u, s, branch and (c_m, c_u) are the restatement's for
    the recorded S_mm, S_uu, S_mu; the recorded cosine is theirs too and meets the generator's stability conditions."""
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    cfg = json.loads(str(g["config"]))
    assert cfg["pareto"] is True and cfg["detach_fused"] is False and cfg["drop_head_uni"] is False
    agreement = 0
    for st in range(cfg["steps"]):
        for e in ("audio", "visual"):
            row = dict(zip(pr.INFO_KEYS, g[f"s{st}.pareto.{e}"]))
            c = pr.coefficients(row["S_mm"], row["S_uu"], row["S_mu"], scale=cfg["pareto_scale"])
            for k in pr.INFO_KEYS:
                assert c[k] == row[k], (st, e, k)
            assert tuple(g[f"s{st}.pareto.{e}.c"]) == (c["c_m"], c["c_u"])
            cos = row["S_mu"] / np.sqrt(row["S_mm"] * row["S_uu"])
            assert cos == float(g[f"s{st}.pareto.{e}.cos"]) and abs(cos) >= 0.05
            raw = float(g[f"s{st}.pareto.{e}.gamma_raw"])
            if row["branch"] == 1:
                agreement += 1
                assert c["gamma_raw"] == raw and (0.05 <= raw <= 0.95 or raw < -0.05 or raw > 1.05)
            else:
                assert np.isnan(raw)
    assert agreement == cfg["agreement_cases"]
