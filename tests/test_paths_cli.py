"""``python -m phasm_amd.cli bubble-paths``: the TSV of every top-level bubble of a graph file.  Without a GPU the lines are
held to the goldens through ``HostPaths``; on the device the command itself runs on graph files written from golden cases
(one segment per two node ids, an ``E`` line per edge in edge order) and must print the same lines."""
import numpy as np
import pytest

import paths_utils as pp
from phasm_amd import cli, phasing
from phasm_amd.io import gfa
from test_paths_oracle import BY_NAME

FILE_CASES = ("direct_two_chains", "direct_saturated_64", "direct_permuted_2", "walk_large_middle", "walk_merged_nodes")


def graph_text(order, edges):
    n_seg = (max(order) >> 1) + 1
    name = lambda x: "s%d%s" % (x >> 1, "+-"[x & 1])   # noqa: E731
    return gfa.gfa_header() + "".join("S\ts%d\t5000\t*\n" % i for i in range(n_seg)) + \
        "".join("E\t*\t%s\t%s\t%d\t5000\t0\t17\t*\n" % (name(u), name(v), w) for u, v, w in edges)


def expected_lines(case, max_bubble_size, listing):
    order, edges, _ = pp.case_inputs(case)
    graph = gfa.read_graph_gfa(graph_text(order, edges).splitlines(True))
    # (the file's node order is the first appearance in its E lines, then the `+` node of every segment without an edge:
    # the case's own order only where that is the same)
    assert set(order) <= {int(x) for x in graph.node_order} and graph.edges[:, :3].tolist() == edges
    bp = phasing.HostPaths(graph.edges, graph.node_order).phase_paths(None, max_bubble_size if listing else 0)
    return list(cli.bubble_paths_lines(graph, bp, max_bubble_size, listing))


def test_the_lines_name_chain_position_ends_interior_paths_and_arm():
    lines = expected_lines(BY_NAME["direct_two_chains"], 1, True)
    assert lines[0] == "#chain\tposition\tentrance\texit\tinterior_nodes\tpaths\tarm\n"
    rows = [ln.rstrip("\n").split("\t") for ln in lines[1:] if not ln.startswith("P")]
    assert [(r[0], r[1], r[5], r[6]) for r in rows] == [("0", "0", "2", "large"), ("0", "1", "2", "large"), ("0", "2", "1", "bare"),
                                                        ("0", "3", "2", "large"), ("0", "4", "2", "large"), ("1", "0", "2", "large"),
                                                        ("1", "1", "2", "large"), ("1", "2", "2", "large")]
    assert rows[0][2:5] == ["s0+", "s1-", "2"]
    listed = [ln for ln in lines if ln.startswith("P")]
    assert listed == ["P\t0\t2\t0\ts3+,s3-\n"]               # only the bare bubble has no more than one path
    lines = expected_lines(BY_NAME["direct_two_chains"], 10, True)
    assert sum(ln.startswith("P") for ln in lines) == 15 and lines[2] == "P\t0\t0\t0\ts0+,s0-,s1-\n"
    sat = expected_lines(BY_NAME["direct_saturated_64"], 10, True)
    assert len(sat) == 2 and sat[1].split("\t")[5:] == [">=2^64-1", "large\n"]
    assert not any(ln.startswith("P") for ln in expected_lines(BY_NAME["direct_two_chains"], 10, False))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FILE_CASES)
def test_the_command_prints_the_lines_of_the_definition(name, tmp_path):
    case = BY_NAME[name]
    order, edges, _ = pp.case_inputs(case)
    path, out = tmp_path / "graph.gfa", tmp_path / "bubbles.tsv"
    path.write_text(graph_text(order, edges))
    for size, listing in ((4, True), (4, False), (1000, True)):
        assert cli.main(["bubble-paths", str(path), "-b", str(size)] + (["--list"] if listing else []) + ["-o", str(out)]) == 0
        assert out.read_text().splitlines(True) == expected_lines(case, size, listing)
    if name.startswith("walk_"):
        rows = [ln.split("\t") for ln in out.read_text().splitlines() if not ln.startswith(("P", "#"))]
        assert np.all([r[6] == "branch" for r in rows])     # (-b 1000: no bubble of a walk is large or bare)
