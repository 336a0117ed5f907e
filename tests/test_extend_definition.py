"""The checker of the inexact extension mode is checked here.

``po_overlaps_ex`` with ``max_diff > 0`` has no reference (the reference overlapper is exact); every GPU test of it
compares with ``oracle/extend_oracle.c``, the build's own restatement.  That restatement is held here against
(1) an independent definition in plain numpy (tests/extend_definition.py: full matrix, band as a mask, ties as tuples)
and (2) rows known by construction (tests/extend_cases.py: cost exactly at max_diff, indel runs exactly at the band,
the canA / canB edges, low-complexity ends that tie, two anchors of a pair without a self-repeat, a candidate list that
overflows the selection table), on every band 0..30 and on seeded fuzz.  With ``max_diff = 0`` the definition is
tied to the reference goldens like the restatement is.  Rows are bit-exact sorted multisets throughout.
"""
import numpy as np
import pytest

import extend_cases as ec
import extend_definition as ed
import golden_utils as gu
from oracle import extend_oracle as eo


def check(case, anchor=32):
    name, seqs, m, max_diff, band, expect = case
    want = ed.overlaps_ex(seqs, m, max_diff, band, anchor)
    got = eo.oracle_overlaps_ex(seqs, m, max_diff, band, anchor)
    assert np.array_equal(got, want), (name, m, max_diff, band, got.tolist()[:6], want.tolist()[:6])
    if expect is not None:
        assert want.tolist() == sorted(list(r) for r in expect), (name, m, max_diff, band, want.tolist(), expect)
    return want


@pytest.mark.parametrize("family", sorted(ec.FAMILIES))
def test_constructed_rows_equal_definition_and_restatement(family):
    cases = ec.constructed_cases(family)
    assert len(cases) >= 8 and all(c[5] is not None for c in cases)
    assert len({len(c[5]) for c in cases}) >= 2 or family == "two_anchors"   # both outcomes (two_anchors: which row, not whether)
    for case in cases:
        assert all(len(s) <= 300 for s in case[1])
        check(case)


def test_two_anchor_pairs_that_both_indexes_take():
    for case in ec.two_anchor_cases(long=True):
        check(case)


def test_selection_overflow_case_reaches_its_path_and_has_its_rows():
    case = ec.overflow_case()
    n_accepted, anchors_of_5 = ec.overflow_preconditions(case, eo.extend_pairs)
    assert n_accepted > 256, n_accepted                               # more than SEL_CAP / 2 of kernels.hip.h
    assert anchors_of_5 == [206, 208]
    check(case)


@pytest.mark.parametrize("eight_bit", [False, True], ids=["2bit", "8bit"])
def test_band_sweep_every_band(eight_bit):
    n_rows = 0
    for W in range(31):
        case = ec.band_sweep_case(W, eight_bit)
        assert all(len(s) <= 300 for s in case[1])
        n_rows += len(check(case, anchor=8 if eight_bit else 32))
    assert n_rows > 31 * 4


def test_fuzz_sets(n_sets=60):
    n_rows = 0
    for t in range(n_sets):
        n_rows += len(check(ec.fuzz_case(t)))
    assert n_rows > 5 * n_sets


def test_definition_with_zero_differences_equals_the_reference_goldens():
    """The pinned half: with max_diff = 0 the definition, too, must be the exact contract (the band is ignored)."""
    n = 0
    for name, seqs, m, want in gu.all_small_cases():
        if max((len(s) for s in seqs), default=0) > 300:
            continue
        assert np.array_equal(ed.overlaps_ex(seqs, m, 0, 5), want), name
        n += 1
    assert n > 400
