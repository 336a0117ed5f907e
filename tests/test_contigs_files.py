"""The writers of the contigs (``layout.write_component_graphs`` on a ``ChainGraph`` that carries contigs), the edge attribute
``contig`` of ``layout.write_graphml``, ``Contigs.path_of`` / ``edges_of`` and the numbering per component, on hand-built
``ChainGraph``s without a GPU: the arrays are those of tests/contig_utils.py in the dataclasses the device route fills, the
GraphML is read back."""
import io
import logging

import numpy as np

import bubblechain_utils as bu
import contig_utils as ct
from phasm_amd import layout
from test_bubblechains_files import EDGES as CHAIN_EDGES, chain_graph, read_graphml
from test_contigs_oracle import as_device

# components 0-2: those of the bubble-chain files (their chain nodes are excluded: what is left of component 0 is the fork
# 14 -> 16, 14 -> 18 behind the chain, of component 1 the fork 32 -> 26, 32 -> 20 in front of its two chains, component 2 is a
# ring); component 3: a tail into a ring with a chord (40 -> 42 -> 44 -> 46 -> 42, 44 -> 42 is no edge; 46 -> 44 is the
# chord); component 4: a node without edges
EDGES = CHAIN_EDGES + [(40, 42), (42, 44), (44, 46), (46, 42), (46, 44)]
N_SEGMENTS = 25


def contig_graph(tmp_path, min_len=0, with_contigs=True, edges=EDGES):
    g, chains, _ = chain_graph(tmp_path, N_SEGMENTS, edges)
    graph = g.graph
    order = [int(n) for n in graph.node_order]
    X = [n for n, c in zip(order, chains["node_chain"].tolist()) if c != bu.NONE]
    lengths = {n: int(graph.node_length(n)) for n in order}
    want = ct.scheme(graph.edges, order, lengths, X, min_len)
    if with_contigs:
        g.contigs = as_device(want, order, graph.edges)
        g.component_contigs = layout.contigs_by_component(g.contigs, g.components)
    return g, want


def subgraph_restated(graph, path):
    """``g.subgraph(path)`` of networkx 1.x: the nodes in path order at first occurrence; per node its out-edges in the
    graph's edge order, those with both ends in the path."""
    nodes = list(dict.fromkeys(path))
    inside = set(nodes)
    edges = [e for n in nodes for e in graph.edges.tolist() if e[0] == n and e[1] in inside]
    return nodes, np.asarray(edges, dtype=np.int64).reshape(-1, 4)


def test_contig_files_names_contents_and_log_lines(tmp_path, caplog):
    g, want = contig_graph(tmp_path)
    graph = g.graph
    assert len(g.components) == 5 and [len(x) for x in g.component_contigs] == [2, 2, 0, 5, 1]
    out = tmp_path / "out"
    with caplog.at_level(logging.INFO, logger=layout.logger.name):
        assert layout.write_component_graphs(str(out), g, ("gfa2", "graphml")) == len(g.components)
    said = [r.getMessage() for r in caplog.records]
    building = "Building contigs not part of a bubble chain..."
    assert said[:7] == ["Connected component 0 with 10 nodes and 11 edges.", "Found bubblechain #0 with 8 nodes and 9 edges", building,
                        "Connected component 1 with 7 nodes and 6 edges.", "Found bubblechain #0 with 3 nodes and 2 edges",
                        "Found bubblechain #1 with 3 nodes and 2 edges", building]
    assert said.count(building) == len(g.components)
    names = sorted(f.name for f in out.iterdir())
    stems = ["component%d" % i for i in range(len(g.components))] + ["component0.bubblechain0", "component1.bubblechain0", "component1.bubblechain1"]
    stems += ["component%d.contig%d" % (i, j) for i, cs in enumerate(g.component_contigs) for j in range(len(cs))]
    assert names == sorted(s + ext for s in stems for ext in (".gfa", ".graphml"))
    for i, cs in enumerate(g.component_contigs):
        marks = {}
        for j, c in enumerate(cs):
            path = g.contigs.path_of(c)
            assert path == ct.path_of(want, graph.edges, c)
            nodes, edges = subgraph_restated(graph, path)
            stem = "component%d.contig%d" % (i, j)
            assert (out / (stem + ".gfa")).read_text() == "".join(layout.component_gfa2_lines(graph, nodes, edges))
            keys, gnodes, gedges = read_graphml((out / (stem + ".graphml")).read_text())
            assert list(gnodes) == [graph.node_name(n) for n in nodes]
            assert [(u, v) for u, v, _ in gedges] == [(graph.node_name(u), graph.node_name(v)) for u, v, _, _ in edges.tolist()]
            assert not any(k[1] in ("contig", "bubblechain") for k in keys.values())
            marks.update({(graph.node_name(a), graph.node_name(b)): str(j) for a, b in zip(path, path[1:])})
        # the component's own GraphML: contig = j on the edges of the reported paths, long; nothing on the others
        keys, gnodes, gedges = read_graphml((out / ("component%d.graphml" % i)).read_text())
        assert keys["d4"] == ("edge", "contig", "long") and keys["d3"] == ("node", "bubblechain", "long")
        assert {(u, v): a.get("contig") for u, v, a in gedges} == {(graph.node_name(u), graph.node_name(v)): marks.get((graph.node_name(u), graph.node_name(v)))
                                                                   for u, v, _, _ in graph.edges[g.components.edges_of(i)].tolist()}
    # component 3: [40, 42] stops at the junction; the ring's path [42, 44] stops at 44 (in-degree 2); [44, 46] ends at the
    # branch, whose two out-edges are late starts; component 4 is the node without edges
    assert [g.contigs.path_of(c) for c in g.component_contigs[3]] == [[40, 42], [42, 44], [44, 46], [46, 42], [46, 44]]
    assert [g.contigs.path_of(c) for c in g.component_contigs[4]] == [[48]]
    assert (out / "component4.contig0.gfa").read_text() == "".join(layout.component_gfa2_lines(graph, [48], graph.edges[:0]))


def test_a_contig_file_holds_every_edge_between_the_nodes_of_the_path(tmp_path):
    # a tail into a ring: the ring's path ends at its first node, which the file holds once
    g, want = contig_graph(tmp_path, edges=[(0, 2), (2, 4), (4, 6), (6, 2)])
    paths = [g.contigs.path_of(c) for c in range(len(g.contigs))]
    assert paths[:2] == [[0, 2], [2, 4, 6, 2]] and all(len(p) == 1 for p in paths[2:])      # (the other segments: nodes without edges)
    nodes, edges = subgraph_restated(g.graph, [2, 4, 6, 2])
    assert nodes == [2, 4, 6] and cu_pairs(edges) == [(2, 4), (4, 6), (6, 2)]
    idx = layout.induced_edges(g.graph.edges, [0, 2])
    assert cu_pairs(g.graph.edges[idx]) == [(0, 2)]
    # [0, 2, 4] on a graph with the extra edges 4 -> 0 and 2 -> 0: every edge between the three nodes, per node in edge order
    e = np.asarray([(4, 0, 1, 1), (0, 2, 1, 1), (2, 4, 1, 1), (2, 0, 1, 1), (4, 8, 1, 1)], dtype=np.int64)
    assert cu_pairs(e[layout.induced_edges(e, [0, 2, 4, 0])]) == [(0, 2), (2, 4), (2, 0), (4, 0)]
    assert len(layout.induced_edges(e, [8])) == 0


def cu_pairs(edges):
    return [(int(x[0]), int(x[1])) for x in np.asarray(edges).reshape(-1, 4).tolist()]


def test_without_contigs_every_file_and_line_is_as_before(tmp_path, caplog):
    g, _ = contig_graph(tmp_path)
    plain, _ = contig_graph(tmp_path, with_contigs=False)
    assert plain.contigs is None and plain.component_contigs is None and plain.bubblechains is not None
    outs = {}
    for tag, x in (("with", g), ("without", plain)):
        out = tmp_path / tag
        caplog.clear()
        with caplog.at_level(logging.INFO, logger=layout.logger.name):
            layout.write_component_graphs(str(out), x, ("gfa2", "graphml"))
        outs[tag] = ({f.name: f.read_text() for f in out.iterdir()}, [r.getMessage() for r in caplog.records])
    files, said = outs["without"]
    with_files, with_said = outs["with"]
    assert not any("contig" in n for n in files) and not any("contigs" in s for s in said)
    assert [s for s in with_said if "contigs" not in s] == said
    for n, text in files.items():
        if n.endswith(".gfa") or "bubblechain" in n:
            assert with_files[n] == text
        else:
            assert "contig" not in text and '<data key="d4">' not in text
            assert '<key id="d4" for="edge" attr.name="contig" attr.type="long" />' in with_files[n]
            assert with_files[n].replace('  <key id="d4" for="edge" attr.name="contig" attr.type="long" />\n', "").count("\n") <= text.count("\n") + \
                with_files[n].count('<data key="d4">')


def test_min_length_drops_contigs_from_the_files_and_renumbers(tmp_path):
    g, want = contig_graph(tmp_path, min_len=1130)
    all_g, all_want = contig_graph(tmp_path)
    assert 0 < want["stats"]["n_contigs"] < all_want["stats"]["n_contigs"] and want["stats"]["n_short_paths"] > 0
    out = tmp_path / "out"
    layout.write_component_graphs(str(out), g, ("graphml",))
    wrote = sorted(f.name for f in out.iterdir() if ".contig" in f.name)
    assert wrote == sorted("component%d.contig%d.graphml" % (i, j) for i, cs in enumerate(g.component_contigs) for j in range(len(cs)))
    for i, cs in enumerate(g.component_contigs):                       # numbered 0.. per component, in contig order
        assert cs == sorted(cs)
        for c in cs:
            assert want["c_length"][c] >= 1130


def test_write_graphml_with_and_without_the_edge_attribute():
    class View:
        node_order, avg_coverage = np.asarray([0, 1]), np.asarray([1.5, 2.5])
        node_name = staticmethod(lambda n: ['a"<+', "b&-"][n])

        def edge_tuples(self):
            return [('a"<+', "b&-", 7, 3), ("b&-", 'a"<+', 8, 4)]

    plain, marked, both = io.StringIO(), io.StringIO(), io.StringIO()
    assert layout.write_graphml(plain, View()) == 2
    assert layout.write_graphml(marked, View(), None, {1: 5}) == 2
    assert layout.write_graphml(both, View(), {"b&-": 4}, {0: 0}) == 2
    assert "contig" not in plain.getvalue() and "d4" not in plain.getvalue()
    none = io.StringIO()
    layout.write_graphml(none, View(), None, None)
    assert none.getvalue() == plain.getvalue()                          # None: today's bytes
    keys, nodes, edges = read_graphml(marked.getvalue())
    assert keys["d4"] == ("edge", "contig", "long") and "d3" not in keys
    assert edges == [('a"<+', "b&-", {"weight": "7", "overlap_len": "3", "avg_coverage": "1.5"}),
                     ("b&-", 'a"<+', {"weight": "8", "overlap_len": "4", "avg_coverage": "2.5", "contig": "5"})]
    keys, nodes, edges = read_graphml(both.getvalue())
    assert nodes == {'a"<+': {}, "b&-": {"bubblechain": "4"}} and edges[0][2]["contig"] == "0" and "contig" not in edges[1][2]
    stripped = marked.getvalue().replace('  <key id="d4" for="edge" attr.name="contig" attr.type="long" />\n', "").replace(
        '      <data key="d4">5</data>\n', "")
    assert stripped == plain.getvalue()
