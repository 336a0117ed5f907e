"""What a rejected po_layout_bubblechains_all / po_layout_contigs_all call says and leaves behind: every PO_ERR_INVALID path
in front of the device with its sentence written out, the outputs untouched; without a GPU a call that passes them returns
PO_ERR_HIP.  An edge end outside the node order never reaches the calls through po_graph_from_edges, which refuses the graph and
writes nothing; behind the ranks the device counts such an edge (tests/test_bubblechains_all_host_emulation.py, for the
kernels)."""
import ctypes

import numpy as np
import pytest

from phasm_amd import _lib
from test_components_rejections import FILL, _have_gpu, from_edges, three_segments
from test_layout_rejections import segment_handle


def chains_call(ov, graph_ptr, min_nodes=1, reserved=0, want_count=True):
    lib = _lib.load()
    bufs = [np.full(64, FILL, dtype=np.uint8) for _ in range(4)]
    n = ctypes.c_uint64(77)
    prm = _lib.PoBubblechainParams(min_nodes, reserved)
    status = lib.po_layout_bubblechains_all(ov._h, graph_ptr, ctypes.byref(prm), *[b.ctypes.data_as(ctypes.c_void_p) for b in bufs],
                                            ctypes.byref(n) if want_count else None)
    return status, lib.po_last_error(ov._h).decode(), bufs, n.value


def contigs_call(ov, graph_ptr, min_nodes=1, reserved=0, want_count=True):
    lib = _lib.load()
    bufs = [np.full(64, FILL, dtype=np.uint8) for _ in range(3)]
    n = ctypes.c_uint64(77)
    prm = _lib.PoContigParams(5000, min_nodes, reserved)
    status = lib.po_layout_contigs_all(ov._h, graph_ptr, ctypes.byref(prm), None, *[b.ctypes.data_as(ctypes.c_void_p) for b in bufs],
                                       ctypes.byref(n) if want_count else None)
    return status, lib.po_last_error(ov._h).decode(), bufs, n.value


def rejected(call, ov, graph, message, min_nodes=1, reserved=0, want_count=True):
    status, said, bufs, n = call(ov, graph._ptr, min_nodes, reserved, want_count)
    assert status == _lib.PO_ERR_INVALID and said == message
    assert all((b == FILL).all() for b in bufs)
    assert n == (0 if want_count else 77)


def test_checks_in_front_of_the_device_keep_their_sentences():
    mine, my_rows = segment_handle("x")
    other, other_rows = segment_handle("y")
    for call, name, counted in ((chains_call, "po_layout_bubblechains_all", "bubble chains"), (contigs_call, "po_layout_contigs_all", "contigs")):
        rejected(call, mine, my_rows, name + ": no room for the number of " + counted, want_count=False)      # a NULL count
        rejected(call, mine, other_rows, name + ": the graph belongs to another handle")                       # a foreign handle
        rejected(call, mine, my_rows, name + ": bad parameters", reserved=1)                                   # reserved != 0
        rejected(call, mine, my_rows, name + ": bad parameters", reserved=3)
        rejected(call, mine, my_rows, name + ": bad parameters", min_nodes=0)                                  # min_nodes == 0
        rejected(call, mine, my_rows, name + " needs an edge result, a merged graph or a po_graph_from_edges result")   # a row result
    with pytest.raises(ValueError, match="bad parameters"):
        mine.layout_bubblechains_all(my_rows, 0, 0)
    with pytest.raises(ValueError, match="32 bits"):
        mine.layout_bubblechains_all(my_rows, 1 << 32, 0)
    with pytest.raises(ValueError, match="bad parameters"):
        mine.layout_contigs_all(my_rows, 5000, 0, None, 0)
    lib = _lib.load()
    n = ctypes.c_uint64()
    assert lib.po_layout_bubblechains_all(mine._h, None, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert lib.po_layout_bubblechains_all(None, my_rows._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert lib.po_layout_contigs_all(mine._h, None, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    st = _lib.PoBubblechainAllStats()
    assert lib.po_get_bubblechain_all_stats(mine._h, None) == _lib.PO_ERR_INVALID
    assert lib.po_get_bubblechain_all_stats(mine._h, ctypes.byref(st)) == _lib.PO_OK and st.n_chains == 0 and st.n_ring_chains == 0
    # the struct: the fields of po_bubblechain_stats, then the additions; 12 x 8 + 8 x 4 + 4 x 4 bytes
    assert ctypes.sizeof(_lib.PoBubblechainAllStats) == 144 and lib.po_abi_version() == 4
    old = [f for f, _ in _lib.PoBubblechainStats._fields_]
    assert [f for f, _ in _lib.PoBubblechainAllStats._fields_ if f in old] == old
    for r in (my_rows, other_rows):
        r.free()
    mine.close()
    other.close()


def test_an_edge_end_outside_the_node_order_writes_nothing():
    from phasm_amd import cyclic
    ov = three_segments()
    status, said, out = from_edges(ov, [(0, 2), (2, 4)], [0, 2])
    assert status == _lib.PO_ERR_INVALID and said == "po_graph_from_edges: an edge has an end that is not in the node order"
    assert out.value is None                                    # no graph result: nothing the calls could be given
    with pytest.raises(ValueError, match="an edge has an end that is not in the node order"):
        cyclic.HostSuperbubblesAll([(0, 2), (2, 4)], [0, 2]).layout_bubblechains_all()
    ov.close()


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_valid_calls_fail_loudly_without_a_gpu():
    ov = three_segments()
    status, _, out = from_edges(ov, [(0, 2)], [0, 2])          # (no graph result without a device ...)
    assert status == _lib.PO_ERR_HIP and out.value is None
    rows = ov.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    status, _, bufs, n = chains_call(ov, rows._ptr)            # (... and a row result is turned away first)
    assert status == _lib.PO_ERR_INVALID and n == 0
    with pytest.raises(Exception):
        ov.layout_bubblechains_all(rows, 1, 0)
    rows.free()
    ov.close()


@pytest.mark.gpu
def test_the_checks_behind_the_device():
    ov = three_segments()
    g = ov.graph_from_edges(np.asarray([[0, 2, 100, 17], [2, 4, 100, 17], [4, 0, 100, 17]]), [4, 2, 0])
    for call, name in ((chains_call, "po_layout_bubblechains_all"), (contigs_call, "po_layout_contigs_all")):
        rejected(call, ov, g, name + ": bad parameters", reserved=3)
        rejected(call, ov, g, name + ": bad parameters", min_nodes=0)
    node_chain, node_bubble, edge_chain, table = ov.layout_bubblechains_all(g)        # a ring of three trivial bubbles, head: rank 0
    assert table.tolist() == [(4, 4, 3, 3, 3)] and node_chain.tolist() == [0, 0, 0] and node_bubble.tolist() == [0, 2, 1]
    assert edge_chain.tolist() == [0, 0, 0]
    node_chain, node_bubble, edge_chain, table = ov.layout_bubblechains_all(g, min_nodes=4)
    assert len(table) == 0 and node_chain.tolist() == node_bubble.tolist() == [_lib.NO_NODE] * 3 and edge_chain.tolist() == [_lib.NO_NODE] * 3
    st = ov.bubblechain_all_stats()
    assert (st["n_short"], st["n_ring_chains"], st["n_ring_bubbles"], st["n_ring_rounds"]) == (1, 1, 3, 3)
    g.free()
    ov.close()
