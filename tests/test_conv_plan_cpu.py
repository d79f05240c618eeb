"""The host-side convolution planner, pinned through the C ABI (no GPU: the queries are host code).

tests/golden/conv_plan.json holds what a build of the commit BEFORE `ConvGeom` (csrc/gather.h) answered for every
convolution of both ResNet18 encoders at the benchmark's input shapes (batch 2 and 64), for the Swin Linears and for a set of
guard geometries (tests/golden/make_golden_conv_plan.py: the sweep, the queries and how the file is recorded).  The internal
interface carries the geometry as one struct with the C ABI's field order; a transposed field anywhere between api.cpp and
the planner changes one of these numbers.  The tuning variables are unset: the fixture is the product's planner."""
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_golden_conv_plan as mk  # noqa: E402

F = mk.FIELDS

# Which recorded geometry tells which pair of fields apart: with the two fields swapped the library answers something else
# than the record, so the record fails if any layer between the C ABI and the planner transposes them.
S2 = (2, 56, 40, 64, 128, 3, 3, 2, 1)         # H != W, 64 -> 128, stride 2, pad 1: no two fields equal but R = S
S2_T = (2, 40, 56, 64, 128, 3, 3, 2, 1)       # its transpose
N3 = (64, 28, 28, 128, 384, 3, 3, 1, 1)       # 128 -> 384: three N-tiles one way, one the other; N = 64 against stride 1
R3S1 = (4, 14, 20, 256, 512, 3, 1, 1, 1)      # 256 -> 512 with a 3x1 filter: R against S, H against W
R1S3 = (4, 14, 20, 256, 512, 1, 3, 1, 1)
SMALL_H = (4, 3, 14, 256, 512, 1, 3, 1, 1)    # a map as small as the filter: H against R ...
SMALL_W = (4, 14, 3, 256, 512, 3, 1, 1, 1)    # ... and W against S
AUDIO1_CREMAD = (2, 65, 47, 64, 64, 3, 3, 1, 1)   # CREMA-D audio layer 1: a channel count against the filter height
AUDIO1_KS = (2, 33, 157, 64, 64, 3, 3, 1, 1)      # Kinetics-Sounds audio layer 1: ... against the filter width
PAIR_GUARDS = {
    ("N", "H"): R1S3, ("N", "W"): N3, ("N", "C"): S2, ("N", "K"): S2, ("N", "R"): S2, ("N", "S"): S2, ("N", "stride"): N3,
    ("N", "pad"): S2,
    ("H", "W"): R3S1, ("H", "C"): S2, ("H", "K"): S2, ("H", "R"): SMALL_H, ("H", "S"): S2_T, ("H", "stride"): S2, ("H", "pad"): S2,
    ("W", "C"): S2, ("W", "K"): S2, ("W", "R"): S2, ("W", "S"): SMALL_W, ("W", "stride"): S2, ("W", "pad"): S2,
    ("C", "K"): N3, ("C", "R"): AUDIO1_CREMAD, ("C", "S"): AUDIO1_KS, ("C", "stride"): S2, ("C", "pad"): S2,
    ("K", "R"): AUDIO1_CREMAD, ("K", "S"): AUDIO1_KS, ("K", "stride"): S2, ("K", "pad"): S2,
    ("R", "S"): R3S1, ("R", "stride"): S2, ("R", "pad"): S2,
    ("S", "stride"): S2, ("S", "pad"): S2,
    ("stride", "pad"): S2,
}
# Beside them the sweep holds the contrasts one geometry cannot: 256 -> 512 at 14 x 20 with stride 1 and 2, with R = 3 (pad 1) and
# R = 1 (pad 0); 128 -> 384 and 384 -> 128; a 3x3 without padding.


@pytest.fixture(scope="module")
def plan():
    assert not os.environ.get("GDL_TUNING"), "the planner fixture is the product's planner: run without GDL_TUNING"
    with open(mk.OUT) as f:
        golden = json.load(f)
    L, lib = mk.load()
    return golden, L, lib


def test_fixture_covers_the_sweep(plan):
    golden, _, _ = plan
    assert tuple(golden["fields"]) == mk.FIELDS and tuple(golden["queries"]) == mk.QUERIES
    assert [tuple(c["g"]) for c in golden["convs"]] == mk.sweep()
    assert len(golden["engines"]) == len(mk.BATCHES) * len(mk.ENGINE_INPUTS) * len(mk.DTYPES)


def test_conv_queries_match_the_recorded_planner(plan):
    golden, L, lib = plan
    bad = []
    for c in golden["convs"]:
        for dt in mk.DTYPES:
            got = mk.query(L, lib, dt, tuple(c["g"]))
            bad += [(dict(zip(F, c["g"])), dt, q, want, have) for q, want, have in zip(mk.QUERIES, c[dt], got) if want != have]
    assert not bad, f"{len(bad)} planner answers differ from the fixture, first: {bad[:5]}"


def test_engine_workspace_matches_the_recorded_plan(plan):
    golden, L, lib = plan
    for e in golden["engines"]:
        got = mk.engine_bytes(L, lib, e["modality"], e["dtype"], e["B"], e["T"], e["H"], e["W"])
        assert got == e["bytes"], e


def test_every_pair_of_fields_has_a_guard(plan):
    """PAIR_GUARDS is complete, its geometries are recorded, and the record of each does tell its pair apart."""
    golden, L, lib = plan
    recorded = {tuple(c["g"]): c for c in golden["convs"]}
    assert set(PAIR_GUARDS) == set(itertools.combinations(F, 2))
    for (a, b), g in PAIR_GUARDS.items():
        i, j = F.index(a), F.index(b)
        s = list(g)
        s[i], s[j] = s[j], s[i]
        assert g in recorded and tuple(s) != g, (a, b)
        # (a swapped channel count below one tile has no weight-gradient plan: that query is left out of the comparison)
        wgrad = min(s[3], s[4]) >= 64
        nq = len(mk.QUERIES) - (0 if wgrad else 1)
        assert any(mk.query(L, lib, dt, tuple(s), wgrad) != recorded[g][dt][:nq] for dt in mk.DTYPES), (a, b, g)
