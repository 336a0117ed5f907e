"""tests/coverage_utils.py -- the plain statement of po_layout_coverage and the scheme the kernels use (per-node sets, then
inclusion-exclusion) -- against every application of tests/golden/coverage_cases.npz, which the reference's own
average_coverage_path produced (tests/golden/make_coverage_golden.py).  Sums, path lengths and quotients are compared with
``==``: no tolerance."""
import numpy as np
import pytest

import coverage_utils as cu
import diamond_utils as du
import merge_utils as mu
import reduce_utils as ru
import tips_utils as tu
from test_diamond_oracle import reduce_flags
from test_merge_oracle import CASES as MERGE_CASES, case_stage1 as merge_case_stage1

GOLDEN = cu.load_golden()
CASES = GOLDEN["cases"]
_MERGE = {c["name"]: c for c in MERGE_CASES}
_TEXT, _APP = {}, {}


def case_stage1(c):
    """(rows, node lengths, stage-1 edges in insertion order, node order) of a case: the cases of merge_cases.npz through
    the cache of tests/test_merge_oracle.py, the seeded cases of tests/coverage_utils.py on their own."""
    if c.get("synth", {}).get("kind") not in cu.SYNTH:
        m = _MERGE[c["name"]]
        return merge_case_stage1(m) + (m["order"],)
    if c["name"] not in _TEXT:
        import layout_utils as lu
        from oracle import layout_oracle as lo
        from phasm_amd.io import gfa
        _, lengths, rows = gfa.read_gfa2_rows(cu.case_text(c).splitlines(True))
        L = lu.node_lengths(lengths)
        got = lo.layout_sequential(rows, L, **c["params"])["edges"]
        e = np.array([[u, v, w, o] for (u, v), (w, o) in got.items()], dtype=np.int64).reshape(-1, 4)
        _TEXT[c["name"]] = (rows, L, e, tu.node_order(rows, L, **c["params"]))
    return _TEXT[c["name"]]


def application(c, r):
    """(rows, edges in (u, v) order, members of the merged nodes, length of every node id) of one recorded application:
    (a) the stage-1 graph, (b) the graph after the restated cleaning chain and merge (computed once)."""
    key = (c["name"], r["stage"])
    if key not in _APP:
        rows, L, e, order = case_stage1(c)
        L = [int(x) for x in L]
        members = {}
        if r["stage"] == "b":
            flags = reduce_flags(_MERGE[c["name"]], e) if c["name"] in _MERGE else None
            _, e, left, _ = du.clean_chain(e, order, reduce_flags=flags)
            m = mu.merge_paths(e, left, L, len(L))
            e = m["edges"]
            members = {len(L) + k: m["members"][m["offsets"][k]:m["offsets"][k + 1]].tolist() for k in range(len(m["lengths"]))}
            L = L + m["lengths"].tolist()
        e = np.asarray(e, dtype=np.int64).reshape(-1, 4)
        _APP[key] = (rows, e[tu.by_uv(e)], members, L)
    return _APP[key]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_statement_and_device_scheme_equal_the_reference(case):
    assert [r["stage"] for r in case["results"]] == ["a", "b"]
    for r in case["results"]:
        rows, e, members, L = application(case, r)
        for fn in (cu.edge_coverage, cu.edge_coverage_by_sets):
            sums, paths, avg = fn(rows, e, members, L)
            cu.check_record(r, e[:, 0], e[:, 1], sums, paths, avg)            # integers with ==, quotients bit for bit
        assert cu.set_stats(rows, e, members) == (r["n_nodes"], r["n_pairs"], r["max_set"])
        # at most one pair per row and direction: the bound the device sizes its table by
        assert r["n_pairs"] <= 2 * len(rows)


def test_every_situation_the_seeded_cases_aim_at_occurs():
    totals = GOLDEN["situation_totals"]
    assert all(totals[s] > 0 for s in cu.SITUATIONS), totals
    names = {c["name"] for c in CASES}
    assert {"_".join(str(v) for v in s.values()) for s in cu.NEW_CASES} <= names


def test_the_quirk_of_a_last_node_of_length_zero_and_the_zero_path():
    """Stage 1 cannot emit an edge into a segment of length 0, so the golden cannot hold one; the
    two restatements agree on what the reference's code does with such an edge: v adds neither length nor reads."""
    rows = [(0, 2, 0, 0, 0, 0), (2, 4, 0, 0, 0, 0), (6, 0, 0, 0, 0, 0)]
    L = [100, 100, 0, 0, 50, 50, 70, 70]
    e = [(0, 2, 30, 1), (2, 4, 5, 1), (2, 2, 7, 1)]
    a = cu.edge_coverage(rows, e, {}, L)
    b = cu.edge_coverage_by_sets(rows, e, {}, L)
    assert a[0].tolist() == b[0].tolist() == [70, 150, 150] and a[1].tolist() == b[1].tolist() == [30, 55, 7]
    with pytest.raises(ZeroDivisionError):
        cu.edge_coverage(rows, [(0, 2, 0, 1)], {}, L)
