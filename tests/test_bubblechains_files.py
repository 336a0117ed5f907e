"""The writers of the bubble chains (``layout.write_component_graphs`` on a ``ChainGraph`` that carries chains) and the node
attribute ``bubblechain`` of ``layout.write_graphml``, on hand-built ``ChainGraph``s without a GPU: the arrays are those of
tests/bubblechain_utils.py in the dataclasses the device route fills, the GraphML is read back."""
import io
import logging
import xml.etree.ElementTree as ET

import numpy as np

import bubblechain_utils as bu
import components_utils as cu
import superbubble_utils as su
from phasm_amd import _lib, layout
from phasm_amd.io import gfa
from test_bubblechains_oracle import as_device

NS = "{http://graphml.graphdrawing.org/xmlns}"


def graph_text(n_segments, edges):
    """A graph file with one S line per segment and one E line per edge (u, v: oriented reads 2i = i+, 2i + 1 = i-)."""
    name = lambda x: "s%d%s" % (x >> 1, "+-"[x & 1])   # noqa: E731
    lines = [gfa.gfa_header()] + [gfa.gfa_line("S", "s%d" % i, 1000 + i, "*") for i in range(n_segments)]
    lines += ["E\t*\t%s\t%s\t%d\t%d\t0\t%d\t*\n" % (name(u), name(v), 100 + k, 1000 + (u >> 1), 17 + k) for k, (u, v) in enumerate(edges)]
    return "".join(lines)


def chain_graph(tmp_path, n_segments, edges, min_nodes=1, with_chains=True):
    """The ChainGraph ``layout.chain_components(path, bubblechains=True)`` builds, from the restatements instead of the device."""
    p = tmp_path / "graph.gfa"
    p.write_text(graph_text(n_segments, edges))
    with open(p) as f:
        graph = gfa.read_graph_gfa(f)
    order = [int(n) for n in graph.node_order]
    weak = cu.weak_components(graph.edges, order)
    table = np.zeros(weak["stats"]["n_components"], dtype=_lib.COMPONENT_DTYPE)
    for k in table.dtype.names:
        table[k] = weak[k]
    comps = layout.Components(np.asarray(order, dtype=np.uint32), weak["node_component"].astype(np.uint32), weak["edge_component"].astype(np.uint32), table, {})
    g = layout.ChainGraph(graph, comps)
    sb = su.scheme(graph.edges, order)
    want = bu.scheme(graph.edges, order, min_nodes, sb)
    if with_chains:
        g.bubblechains = as_device(want, order, sb)
        g.component_chains = layout.chains_by_component(g.bubblechains, comps)
    return g, want, weak


# component 0: diamond, edge, diamond, then a fork that is no bubble (one chain of 3 bubbles, 8 nodes, 9 edges; 2 nodes in
# none); component 1: two chains joined by a fork; component 2: a 3-cycle (no chain)
D = su._diamond
EDGES = D(0, 2, 4, 6) + [(6, 8)] + D(8, 10, 12, 14) + [(14, 16), (14, 18)] + \
    [(32, 26), (32, 20), (26, 28), (28, 30), (20, 22), (22, 24)] + [(34, 36), (36, 38), (38, 34)]


def read_graphml(text):
    root = ET.fromstring(text)
    keys = {k.get("id"): (k.get("for"), k.get("attr.name"), k.get("attr.type")) for k in root.iter(NS + "key")}
    nodes = {}
    for n in root.iter(NS + "node"):
        nodes[n.get("id")] = {keys[d.get("key")][1]: d.text for d in n.iter(NS + "data")}
        assert all(keys[d.get("key")][0] == "node" for d in n.iter(NS + "data"))
    edges = []
    for e in root.iter(NS + "edge"):
        assert all(keys[d.get("key")][0] == "edge" for d in e.iter(NS + "data"))
        edges.append((e.get("source"), e.get("target"), {keys[d.get("key")][1]: d.text for d in e.iter(NS + "data")}))
    return keys, nodes, edges


def test_chain_files_names_contents_and_log_lines(tmp_path, caplog):
    g, want, weak = chain_graph(tmp_path, 20, EDGES)
    graph = g.graph
    assert len(g.components) == 3 and [len(x) for x in g.component_chains] == [1, 2, 0]
    assert want["c_nodes"].tolist() == [8, 3, 3] and want["c_edges"].tolist() == [9, 2, 2] and want["c_bubbles"].tolist() == [3, 2, 2]
    out = tmp_path / "out"
    with caplog.at_level(logging.INFO, logger=layout.logger.name):
        assert layout.write_component_graphs(str(out), g, ("gfa2", "graphml")) == 3
    said = [r.getMessage() for r in caplog.records]
    assert said == ["Connected component 0 with 10 nodes and 11 edges.", "Found bubblechain #0 with 8 nodes and 9 edges",
                    "Connected component 1 with 7 nodes and 6 edges.", "Found bubblechain #0 with 3 nodes and 2 edges",
                    "Found bubblechain #1 with 3 nodes and 2 edges", "Connected component 2 with 3 nodes and 3 edges."]
    names = sorted(f.name for f in out.iterdir())
    stems = ["component0", "component0.bubblechain0", "component1", "component1.bubblechain0", "component1.bubblechain1", "component2"]
    assert names == sorted(s + ext for s in stems for ext in (".gfa", ".graphml"))
    bc = g.bubblechains
    for i, chains in enumerate(g.component_chains):
        for j, c in enumerate(chains):
            nodes, edges = bc.nodes_of(c).tolist(), graph.edges[bc.edges_of(c)]
            assert nodes == bu.nodes_of(want, graph.node_order, c)
            stem = "component%d.bubblechain%d" % (i, j)
            assert (out / (stem + ".gfa")).read_text() == "".join(layout.component_gfa2_lines(graph, nodes, edges))   # the existing writer
            keys, gnodes, gedges = read_graphml((out / (stem + ".graphml")).read_text())
            assert list(gnodes) == [graph.node_name(n) for n in nodes] and all(a == {} for a in gnodes.values())
            assert [(u, v) for u, v, _ in gedges] == [(graph.node_name(u), graph.node_name(v)) for u, v, _, _ in edges.tolist()]
            assert [(int(a["weight"]), int(a["overlap_len"])) for _, _, a in gedges] == [(w, o) for _, _, w, o in edges.tolist()]
            assert not any(k[1] == "bubblechain" for k in keys.values())
    # the component's own GraphML: bubblechain = j on the chain's nodes, long; nothing on the others
    for i in range(3):
        keys, gnodes, gedges = read_graphml((out / ("component%d.graphml" % i)).read_text())
        assert ("node", "bubblechain", "long") in keys.values()
        marks = {}
        for j, c in enumerate(g.component_chains[i]):
            marks.update({graph.node_name(n): str(j) for n in bc.nodes_of(c).tolist()})
        assert {n: a.get("bubblechain") for n, a in gnodes.items()} == {graph.node_name(n): marks.get(graph.node_name(n))
                                                                        for n in g.components.nodes_of(i).tolist()}
        assert len(gedges) == len(g.components.edges_of(i))
    assert sum(1 for a in read_graphml((out / "component0.graphml").read_text())[1].values() if a) == 8
    assert sum(1 for a in read_graphml((out / "component2.graphml").read_text())[1].values() if a) == 0
    # the second chain of component 1 is the second by the rank of its head
    assert bc.bubbles_of(g.component_chains[1][0])[0][0] == 26 and bc.bubbles_of(g.component_chains[1][1])[0][0] == 20


def test_without_chains_every_file_and_line_is_as_before(tmp_path, caplog):
    g, _, _ = chain_graph(tmp_path, 20, EDGES)
    plain, _, _ = chain_graph(tmp_path, 20, EDGES, with_chains=False)
    assert plain.bubblechains is None and plain.component_chains is None
    outs = {}
    for tag, x in (("with", g), ("without", plain)):
        for fmt in (("gfa1",), ("gfa2", "graphml")):
            out = tmp_path / (tag + fmt[0])
            caplog.clear()
            with caplog.at_level(logging.INFO, logger=layout.logger.name):
                layout.write_component_graphs(str(out), x, fmt)
            outs[tag, fmt[0]] = ({f.name: f.read_text() for f in out.iterdir()}, [r.getMessage() for r in caplog.records])
    for fmt in ("gfa1", "gfa2"):
        files, said = outs["without", fmt]
        assert sorted(files) == sorted("component%d.%s" % (i, e) for i in range(3) for e in (("gfa",) if fmt == "gfa1" else ("gfa", "graphml")))
        assert said == ["Connected component 0 with 10 nodes and 11 edges.", "Connected component 1 with 7 nodes and 6 edges.",
                        "Connected component 2 with 3 nodes and 3 edges."]
        with_files = outs["with", fmt][0]
        assert all(with_files[n] == text for n, text in files.items() if n.endswith(".gfa"))      # the component's GFA is untouched
        for n, text in files.items():
            if n.endswith(".graphml"):
                assert "bubblechain" not in text and "<data key=\"d3\">" not in text
                view = layout._ComponentView(plain.graph, plain.components.nodes_of(int(n[9])).tolist(),
                                             plain.graph.edges[plain.components.edges_of(int(n[9]))])
                buf = io.StringIO()
                layout.write_graphml(buf, view)                                                 # no attribute asked for: today's bytes
                assert buf.getvalue() == text
                assert '<key id="d3" for="node" attr.name="bubblechain" attr.type="long" />' in with_files[n]


def test_min_nodes_drops_chains_from_the_files(tmp_path):
    g, want, _ = chain_graph(tmp_path, 20, EDGES, min_nodes=4)
    assert want["stats"]["n_short"] == 2 and [len(x) for x in g.component_chains] == [1, 0, 0]
    out = tmp_path / "out"
    layout.write_component_graphs(str(out), g, ("graphml",))
    assert sorted(f.name for f in out.iterdir()) == ["component0.bubblechain0.graphml", "component0.graphml", "component1.graphml",
                                                     "component2.graphml"]
    _, gnodes, _ = read_graphml((out / "component1.graphml").read_text())
    assert len(gnodes) == 7 and not any(gnodes.values())


def test_write_graphml_escapes_names_beside_the_attribute():
    class View:
        node_order, avg_coverage = np.asarray([0, 1]), np.asarray([1.5])
        node_name = staticmethod(lambda n: ['a"<+', "b&-"][n])

        def edge_tuples(self):
            return [('a"<+', "b&-", 7, 3)]

    buf = io.StringIO()
    assert layout.write_graphml(buf, View(), {"b&-": 4}) == 1
    keys, nodes, edges = read_graphml(buf.getvalue())
    assert nodes == {'a"<+': {}, "b&-": {"bubblechain": "4"}} and keys["d3"] == ("node", "bubblechain", "long")
    assert edges == [('a"<+', "b&-", {"weight": "7", "overlap_len": "3", "avg_coverage": "1.5"})]
