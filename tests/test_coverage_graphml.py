"""layout.write_graphml and the coverage fields of AssemblyEdges without a GPU: the file parses, carries exactly the graph's
nodes, edges and three attributes (names that need escaping included), and reads back to the doubles that were written."""
import io
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from phasm_amd import _lib, layout


def graph():
    e = np.zeros(3, dtype=_lib.EDGE_DTYPE)
    e["u"], e["v"], e["weight"], e["overlap_len"] = [0, 2, 4], [2, 4, 4], [5, 7, -3], [9, 8, 7]
    g = layout.AssemblyEdges(e, None, ["a+", "a-", "b<&\"+", "b<&\"-"], {})
    g.merged_paths = (np.array([0, 2]), np.array([1, 3]), np.array([3, 0]), np.array([77]))
    g.node_order, g.node_lengths = np.array([2, 0, 4]), np.array([10, 10, 10, 10])
    g.coverage_sums = np.zeros(3, dtype=_lib.COVERAGE_DTYPE)
    g.coverage_sums["read_length_sum"], g.coverage_sums["path_length"] = [10, 1, 6000000000], [3, 3, 7]
    g.avg_coverage = layout._quotients(g.coverage_sums)
    return g


def test_graphml_carries_the_graph_and_reads_back_bit_for_bit():
    g = graph()
    f = io.StringIO()
    assert layout.write_graphml(f, g) == 3
    ns = "{http://graphml.graphdrawing.org/xmlns}"
    root = ET.fromstring(f.getvalue().encode())
    keys = {k.get("id"): (k.get("attr.name"), k.get("attr.type")) for k in root.iter(ns + "key")}
    assert sorted(keys.values()) == [("avg_coverage", "double"), ("overlap_len", "long"), ("weight", "long")]
    assert [n.get("id") for n in root.iter(ns + "node")] == ["b<&\"+", "a+", "merged0+"]           # the node order
    got = {(x.get("source"), x.get("target")): {keys[d.get("key")][0]: d.text for d in x.iter(ns + "data")} for x in root.iter(ns + "edge")}
    want = {(u, v): {"weight": str(w), "overlap_len": str(o), "avg_coverage": repr(c)}
            for (u, v, w, o), c in zip(g.edge_tuples(), g.avg_coverage.tolist())}
    assert got == want and [float(x["avg_coverage"]) for x in got.values()] == [10 / 3, 1 / 3, 6000000000 / 7]
    networkx = pytest.importorskip("networkx")
    back, mine = networkx.read_graphml(io.BytesIO(f.getvalue().encode())), g.to_networkx()
    assert {(u, v): d for u, v, d in back.edges(data=True)} == {(u, v): d for u, v, d in mine.edges(data=True)}
    assert all(set(d) == {"weight", "overlap_len", "avg_coverage"} for _, _, d in mine.edges(data=True))


def test_without_coverage_nothing_is_added_and_a_zero_path_raises():
    g = graph()
    g.avg_coverage = g.coverage_sums = None
    f = io.StringIO()
    layout.write_graphml(f, g)
    assert "avg_coverage" not in f.getvalue()
    sums = np.zeros(2, dtype=_lib.COVERAGE_DTYPE)
    sums["read_length_sum"], sums["path_length"] = [6, 5], [4, 0]
    with pytest.raises(ZeroDivisionError):
        layout._quotients(sums)
    pytest.importorskip("networkx")
    assert all(set(d) == {"weight", "overlap_len"} for _, _, d in g.to_networkx().edges(data=True))
