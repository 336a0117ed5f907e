"""po_overlaps_ex with max_diff > 0 at its edges: the three DP mappings of phasm_amd/csrc/extend.hip.h and the longest-only
selection of kernels.hip.h on the deterministic cases of tests/extend_cases.py.

The mode has no reference (the reference overlapper is exact).  The rows must equal the CPU restatement
(oracle/extend_oracle.c, run in the checker process), which tests/test_extend_definition.py holds against an independent
definition on exactly these cases; and where a case's rows are known by construction they must equal those too.  What the
cases reach that seeded noise does not: every band 0..30 on 2-bit and 8-bit reads; a cost exactly at max_diff and one above;
an indel run exactly as long as the band and one longer; rem = lb + W against lb + W + 1 (and the mirror); differences on
the rows where k_extend_bits changes from single rows to blocks of 16 and rounds of 64; all differences ahead of the first
band-minimum test; end rows inside homopolymers and (AC)n arrays, where many cells tie; two accepted anchors of a pair
whose b does not repeat its prefix; a candidate list with more accepted A candidates than the selection's LDS table takes.
Every call asserts from the stats which mapping ran.  Bit-exact rows, sorted multisets.
"""
import numpy as np
import pytest

import checker as ck
import extend_cases as ec
from oracle import overlap_oracle as oo   # row helpers only
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

CHUNK = 40   # constructed cases per test


@pytest.fixture(params=["bits", "lanes", "wave"], autouse=True)
def dp_kernel(request, monkeypatch):
    """The fixture of tests/test_gpu_extend.py: every test runs through all three mappings of the DP; where a lane mapping
    does not apply (band > 15, 8-bit reads) the library picks the wave kernel by itself."""
    if request.param == "wave":
        monkeypatch.setenv("PHASM_DP_KERNEL", "wave")
    elif request.param == "lanes":
        monkeypatch.setenv("PHASM_DP_SORT", "1")
        monkeypatch.setenv("PHASM_DP_KERNEL_SOFT", "lanes")
    else:
        monkeypatch.delenv("PHASM_DP_KERNEL", raising=False)
        monkeypatch.setenv("PHASM_DP_SORT", "1")
    return request.param


def ex_rows(seqs, m, max_diff, band):
    guard = ck.GuardedReads(seqs)
    ov = ExactOverlapper()
    guard.add_all(ov)
    arr = ov.overlaps_ex_array(m, max_diff, band)
    st = ov.stats()
    ov.close()
    guard.verify_and_close()
    return oo.sort_rows(oo.struct_to_rows(arr)), st


def run_case(case, dp_kernel, bits=2):
    name, seqs, m, max_diff, band, expect = case
    assert max_diff > 0
    got, st = ex_rows(seqs, m, max_diff, band)
    want = ck.oracle_overlaps_ex(seqs, m, max_diff, band, anchor=32 if bits == 2 else 8)
    ctx = (name, dp_kernel, m, max_diff, band)
    # which mapping ran: no case passes by falling back.  (A fuzz set without a single anchor launches no DP at all; every
    # constructed case has its anchor.)
    lane_mapping = dp_kernel != "wave" and band <= 15 and bits == 2 and st["n_candidates"] > 0
    assert st["n_candidates"] > 0 or (expect is None and len(want) == 0), ctx
    assert st["dp_lanes"] == ((2 if dp_kernel == "bits" else 1) if lane_mapping else 0), (ctx, st["dp_lanes"])
    assert st["bits_per_base"] == bits and st["paired"] == 0 and st["max_diff"] == max_diff and st["band"] == band, ctx
    # the mode is defined on the narrow index's anchors (b's prefix K-mer); the wide index anchors a pair elsewhere in b and lists
    # other candidates once there are differences: an inexact call never takes it, whatever its size or PHASM_INDEX
    assert st["wide_index"] == 0, ctx
    assert np.array_equal(got, want), (ctx, len(got), len(want), got.tolist()[:6], want.tolist()[:6])
    if expect is not None:
        assert got.tolist() == sorted(list(r) for r in expect), (ctx, got.tolist(), expect)
    return got


_CASES = {f: ec.constructed_cases(f) for f in ec.FAMILIES}
_CHUNKS = [(f, k) for f in sorted(_CASES) for k in range(0, len(_CASES[f]), CHUNK)]


@pytest.mark.parametrize("family,first", _CHUNKS, ids=["%s%d" % (f, k // CHUNK) for f, k in _CHUNKS])
def test_constructed_cases(family, first, dp_kernel):
    """Two reads each; rows known by construction (the builder says why), equal to the restatement's."""
    for case in _CASES[family][first:first + CHUNK]:
        run_case(case, dp_kernel)


@pytest.mark.parametrize("index", ["narrow", "wide"])
def test_two_anchors_without_a_self_repeat_under_both_indexes(index, dp_kernel, monkeypatch):
    """Two accepted A candidates of one (a, b) whose b does NOT repeat its prefix K-mer -- impossible in the exact mode, where
    the selection's shortcut comes from: the row of the longer overlap only, whichever index was asked for.  (Regression:
    the wide index found the pair through b's K-mer at offset (-p) mod 32, which the two extra bases of the longer overlap
    put out of phase -- the candidate at p = 40 was never listed and the row of p = 42 came out.)"""
    monkeypatch.setenv("PHASM_INDEX", index)
    for case in ec.two_anchor_cases(long=True):
        run_case(case, dp_kernel)


@pytest.mark.parametrize("index", ["narrow", "wide"])
def test_selection_overflow_with_differences(index, dp_kernel, monkeypatch):
    """A list with more accepted A candidates than the selection's LDS table takes goes to the global (a, b) table; in the same
    list stands a b with two accepted anchors that does not repeat its prefix."""
    case = ec.overflow_case()
    extend_pairs = lambda *args: ck.sidecar().call("oracle.extend_oracle", "extend_pairs", *args)   # noqa: E731
    n_accepted, anchors_of_5 = ec.overflow_preconditions(case, extend_pairs)
    assert n_accepted > 256, n_accepted          # SEL_CAP / 2 of kernels.hip.h
    assert len(anchors_of_5) == 2, anchors_of_5
    monkeypatch.setenv("PHASM_INDEX", index)
    run_case(case, dp_kernel)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("bits", [2, 8])
def test_band_sweep(bits, half, dp_kernel):
    """Every band 0..30, one call each, on twelve reads of random and tandem sequence; 2-bit and 8-bit stores."""
    n_rows = 0
    for W in range(16 * half, min(16 * half + 16, 31)):
        n_rows += len(run_case(ec.band_sweep_case(W, eight_bit=bits == 8), dp_kernel, bits=bits))
    assert n_rows > 15 * 4


@pytest.mark.parametrize("third", [0, 1, 2])
def test_fuzz_sets(third, dp_kernel):
    for t in range(20 * third, 20 * third + 20):
        run_case(ec.fuzz_case(t), dp_kernel)
