"""The files of ``chain-components --bubblechains --cyclic`` / ``chain --cyclic`` for a ring component, from the existing
writers (``layout.write_component_graphs``), on hand-built ``ChainGraph``s without a GPU: the arrays are those of
tests/bubblechain_all_utils.py in the dataclasses the device route fills, in the pattern of tests/test_bubblechains_files.py."""
import logging

import numpy as np

import bubblechain_all_utils as ba
import components_utils as cu
import contig_utils as ct
import cyclic_utils as cy
from phasm_amd import _lib, layout
from phasm_amd.io import gfa
from test_bubblechains_files import graph_text, read_graphml
from test_bubblechains_oracle import as_device
from test_contigs_oracle import as_device as contigs_as_device

D = cy._diamond
# component 0: a ring of three diamonds (9 nodes, 12 edges); component 1: a path chain of two diamonds and a fork that is no bubble
RING = [e for i in range(3) for e in D(6 * i, 6 * i + 2, 6 * i + 4, 6 * ((i + 1) % 3))]
EDGES = RING + D(18, 20, 22, 24) + D(24, 26, 28, 30) + [(30, 32), (30, 34)]


def chain_graph(tmp_path, n_segments, edges, min_nodes=1, cyclic=True, contigs=False):
    """The ChainGraph ``layout.chain_components(path, bubblechains=True, cyclic=cyclic)`` builds, from the restatements."""
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
    if cyclic:
        sb = cy.scheme_all(graph.edges[:, :2].tolist(), order)
        want = ba.scheme(graph.edges, order, min_nodes)
    else:
        import bubblechain_utils as bu
        import superbubble_utils as su
        sb = su.scheme(graph.edges, order)
        want = bu.scheme(graph.edges, order, min_nodes, sb)
    g.bubblechains = as_device(want, order, sb)
    g.component_chains = layout.chains_by_component(g.bubblechains, comps)
    if contigs:
        lengths = {n: int(graph.node_length(n)) for n in order}
        X = [n for n, c in zip(order, want["node_chain"].tolist()) if c != ba.NONE]
        g.contigs = contigs_as_device(ct.scheme(graph.edges, order, lengths, X, 0), order, graph.edges)
        g.component_contigs = layout.contigs_by_component(g.contigs, comps)
    return g, want


def test_a_ring_component_is_one_chain_file_that_holds_every_node(tmp_path, caplog):
    g, want = chain_graph(tmp_path, 18, EDGES)
    graph = g.graph
    assert len(g.components) == 2 and [len(x) for x in g.component_chains] == [1, 1]
    assert want["c_first"].tolist() == want["c_last"].tolist()[:1] + [18] and want["c_bubbles"].tolist() == [3, 2]
    assert want["c_nodes"].tolist() == [9, 7] and want["c_edges"].tolist() == [12, 8] and want["stats"]["n_ring_chains"] == 1
    out = tmp_path / "out"
    with caplog.at_level(logging.INFO, logger=layout.logger.name):
        assert layout.write_component_graphs(str(out), g, ("gfa2", "graphml")) == 2
    said = [r.getMessage() for r in caplog.records]
    assert said == ["Connected component 0 with 9 nodes and 12 edges.", "Found bubblechain #0 with 9 nodes and 12 edges",
                    "Connected component 1 with 9 nodes and 10 edges.", "Found bubblechain #0 with 7 nodes and 8 edges"]
    stems = ["component0", "component0.bubblechain0", "component1", "component1.bubblechain0"]
    assert sorted(f.name for f in out.iterdir()) == sorted(s + ext for s in stems for ext in (".gfa", ".graphml"))
    bc = g.bubblechains
    ring = g.component_chains[0][0]
    nodes, edges = bc.nodes_of(ring).tolist(), graph.edges[bc.edges_of(ring)]
    assert nodes == g.components.nodes_of(0).tolist() and len(edges) == 12             # the whole component
    assert (out / "component0.bubblechain0.gfa").read_text() == "".join(layout.component_gfa2_lines(graph, nodes, edges))   # the existing writer
    assert (out / "component0.bubblechain0.gfa").read_text() == (out / "component0.gfa").read_text()
    walk = bc.bubbles_of(ring)
    assert walk == [(0, 6), (6, 12), (12, 0)]                                            # once round, from the lowest-ranked entrance
    keys, gnodes, gedges = read_graphml((out / "component0.graphml").read_text())
    assert ("node", "bubblechain", "long") in keys.values() and all(a.get("bubblechain") == "0" for a in gnodes.values()) and len(gnodes) == 9


def test_without_the_flag_the_ring_component_has_no_chain(tmp_path):
    """What the acyclic route gives on the same file: 0 chains in the ring component -- the state this feature ends."""
    g, want = chain_graph(tmp_path, 18, EDGES, cyclic=False)
    assert [len(x) for x in g.component_chains] == [0, 1] and want["c_first"].tolist() == [18]
    out = tmp_path / "out"
    layout.write_component_graphs(str(out), g, ("gfa2",))
    assert sorted(f.name for f in out.iterdir()) == ["component0.gfa", "component1.bubblechain0.gfa", "component1.gfa"]


def test_no_contig_is_cut_out_of_the_ring(tmp_path):
    g, want = chain_graph(tmp_path, 18, EDGES, contigs=True)
    out = tmp_path / "out"
    layout.write_component_graphs(str(out), g, ("gfa2",))
    names = sorted(f.name for f in out.iterdir())
    assert not any(n.startswith("component0.contig") for n in names) and "component0.bubblechain0.gfa" in names
    assert [n for n in names if ".contig" in n] == ["component1.contig0.gfa", "component1.contig1.gfa"]      # the fork behind the path chain
    assert [g.contigs.path_of(j) for j in g.component_contigs[1]] == [[30, 32], [30, 34]]


def test_min_nodes_drops_the_ring_from_the_files(tmp_path):
    g, want = chain_graph(tmp_path, 18, EDGES, min_nodes=8)
    assert (want["stats"]["n_short"], want["stats"]["n_ring_chains"]) == (1, 1) and [len(x) for x in g.component_chains] == [1, 0]
    g, want = chain_graph(tmp_path, 18, EDGES, min_nodes=10)
    assert want["stats"]["n_short"] == 2 and [len(x) for x in g.component_chains] == [0, 0]
