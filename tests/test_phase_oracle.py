"""The restated loops of the reference (``definition``) and the table decomposition the device uses (``scheme``) against
tests/golden/phase_cases.npz, which tests/golden/make_phase_golden.py recorded from the reference's own ``branch``, ``prune`` and
``phase_large_bubble``; ``prune_levels`` against the reference's float accumulation of the prune factor."""
import math

import pytest

import phase_utils as pu
from phasm_amd import phasing

GOLDEN = pu.load_golden()
CASES = GOLDEN["cases"]
NAMES = [c["name"] for c in CASES]


def case_of(name):
    return next(c for c in CASES if c["name"] == name)


def test_the_golden_holds_every_spec_and_every_situation():
    assert NAMES == list(pu.SPECS)
    seen = set()
    for c in CASES:
        seen |= set(c["situations"])
        spec = pu.SPECS[c["name"]]
        assert (c["k"], c["P"], c["C"], c["R"], c["n_b"], c["start"]) == tuple(spec[x] for x in ("k", "P", "C", "R", "n_b", "start"))
    assert seen == set(pu.SITUATIONS)
    # the shapes the kernels branch on: bitset words, wave / workgroup / tile of the reduction, ploidies, path counts, candidates
    assert {1, 31, 32, 33, 65} <= {c["n_b"] for c in CASES}
    assert {0, 1, 2, 63, 64, 65, 257, 2049} <= {c["R"] for c in CASES}
    assert {(1, 64), (2, 64), (8, 2)} <= {(c["k"], c["P"]) for c in CASES} and {1, 2, 3, 4, 8} <= {c["k"] for c in CASES}
    assert {1, 2, 10, 64} <= {c["P"] for c in CASES} and {1, 2, 65} <= {c["C"] for c in CASES}
    assert {0, 1} == {c["start"] for c in CASES}
    assert GOLDEN["worst_scheme_difference"] < 1e-14


@pytest.mark.parametrize("name", NAMES)
def test_definition_equals_the_reference(name):
    case = case_of(name)
    all_rl = []
    got = pu.definition(case, all_rl)
    pu.check_result(got, case["ref"], case, exact_rl=True)      # the same loops in the same order: the same bits
    assert got["levels"] == case["ref"]["levels"]
    assert sorted(pu.situations(case, case["ref"], all_rl)) == case["situations"]
    assert pu.conditions_hold(case, [x[2] for x in all_rl], case["ref"]["kept_rl"], case["ref"]["levels"], case["ref"]["scores"])


@pytest.mark.parametrize("name", NAMES)
def test_scheme_equals_the_reference(name):
    case = case_of(name)
    got = pu.scheme(case)
    pu.check_result(got, case["ref"], case)
    assert got["level_used"] == (len(case["ref"]["levels"]) - 1 if case["ref"]["levels"] else -1)
    assert got["surv_rl"] == [got["kept_rl"][j] for j in got["surv"]]


def test_prune_levels_is_the_reference_accumulation():
    seqs = GOLDEN["level_sequences"]
    assert len(seqs) >= 8
    for s in seqs:
        assert phasing.prune_levels(s["factor"], s["step"], s["max_rounds"]) == s["levels"]
    first = seqs[0]   # 0.1 + 9 * 0.1 in float stays below 1.0: the loop runs once more and the last level is above 0
    assert (first["factor"], first["step"]) == (0.1, 0.1) and len(first["levels"]) == 11
    assert first["levels"][9] == math.log10(0.9999999999999999) < 0.0 < first["levels"][10]
    assert any(s["factor"] < 1.0 and s["levels"] and s["levels"][-1] > 0.0 and len(s["levels"]) < s["max_rounds"] for s in seqs)
    assert phasing.prune_levels(0.0, 0.1, 9) == [] and phasing.prune_levels(-1.0, 0.1, 9) == []
    assert phasing.prune_levels(0.5, 0.1, 1) == [math.log10(0.5)] and phasing.prune_levels(1.0, 0.1, 9) == [0.0]


def test_the_big_case_meets_the_conditions_too():
    case = pu.build(pu.BIG_SPEC)
    assert case["C"] * case["P"] ** case["k"] == 530000 > 524288
