"""What a rejected po_layout_components or po_graph_from_edges call says and leaves behind: every PO_ERR_INVALID path with
its sentence written out, the outputs untouched.  The checks of po_graph_from_edges run on the host before anything
touches the device, so they are held here without a GPU; a VALID call without a GPU returns PO_ERR_HIP.  The five
existing stages refuse a graph that did not come from po_layout_edges with the sentences they have always used."""
import ctypes

import numpy as np
import pytest

from phasm_amd import _lib
from phasm_amd.overlapper import ExactOverlapper
from test_layout_rejections import STAGES, coverage_rejected, rejected, segment_handle

FILL = 0xAB


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def components_call(ov, graph_ptr, reserved=0, want_count=True):
    lib = _lib.load()
    bufs = [np.full(64, FILL, dtype=np.uint8) for _ in range(3)]
    n = ctypes.c_uint64(77)
    prm = _lib.PoComponentsParams(reserved)
    status = lib.po_layout_components(ov._h, graph_ptr, ctypes.byref(prm), *[b.ctypes.data_as(ctypes.c_void_p) for b in bufs],
                                      ctypes.byref(n) if want_count else None)
    return status, lib.po_last_error(ov._h).decode(), bufs, n.value


def components_rejected(ov, graph, message, reserved=0, want_count=True):
    status, said, bufs, n = components_call(ov, graph._ptr, reserved, want_count)
    assert status == _lib.PO_ERR_INVALID and said == message
    assert all((b == FILL).all() for b in bufs)
    assert n == (0 if want_count else 77)


def from_edges(ov, edges, order):
    lib = _lib.load()
    e = np.zeros(len(edges), dtype=_lib.EDGE_DTYPE)
    for k, (u, v) in enumerate(edges):
        e[k] = (u, v, 100, 17)
    o = np.asarray(order, dtype=np.uint32)
    out = ctypes.c_void_p()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if len(a) else None   # noqa: E731
    status = lib.po_graph_from_edges(ov._h, ptr(e), len(e), ptr(o), len(o), ctypes.byref(out))
    return status, lib.po_last_error(ov._h).decode(), out


def three_segments():
    ov = ExactOverlapper()
    for name in "abc":
        ov.add_segment(name, 10)
    return ov


def test_components_checks_in_front_of_the_device_keep_their_sentences():
    mine, my_rows = segment_handle("x")
    other, other_rows = segment_handle("y")
    components_rejected(mine, my_rows, "po_layout_components: no room for the number of components", want_count=False)
    components_rejected(mine, other_rows, "po_layout_components: the graph belongs to another handle")
    components_rejected(mine, my_rows, "po_layout_components: bad parameters", reserved=1)
    components_rejected(mine, my_rows, "po_layout_components needs an edge result, a merged graph or a po_graph_from_edges result")
    lib = _lib.load()
    n = ctypes.c_uint64()
    assert lib.po_layout_components(mine._h, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert lib.po_layout_components(None, my_rows._ptr, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    for r in (my_rows, other_rows):
        r.free()
    mine.close()
    other.close()


@pytest.mark.parametrize("edges, order, message", [
    ([(0, 6)], [0, 6], "po_graph_from_edges: the node order names a read the handle does not hold"),
    ([(0, 2)], [0, 2, 0], "po_graph_from_edges: a node appears twice in the node order"),
    ([(0, 7)], [0, 2], "po_graph_from_edges: an edge names a read the handle does not hold"),
    ([(6, 0)], [0, 2], "po_graph_from_edges: an edge names a read the handle does not hold"),
    ([(0, 2), (2, 4)], [0, 2], "po_graph_from_edges: an edge has an end that is not in the node order"),
    ([(4, 2)], [0, 2], "po_graph_from_edges: an edge has an end that is not in the node order"),
    ([(0, 2), (2, 0), (0, 2)], [0, 2], "po_graph_from_edges: an edge appears twice"),
], ids=["order_out_of_range", "order_twice", "v_out_of_range", "u_out_of_range", "v_not_in_order", "u_not_in_order", "edge_twice"])
def test_graph_from_edges_host_checks(edges, order, message):
    ov = three_segments()
    status, said, out = from_edges(ov, edges, order)
    assert status == _lib.PO_ERR_INVALID and said == message and out.value is None
    ov.close()


def test_graph_from_edges_null_arguments():
    ov = three_segments()
    lib = _lib.load()
    out = ctypes.c_void_p()
    order = np.asarray([0, 2], dtype=np.uint32)
    assert lib.po_graph_from_edges(ov._h, None, 1, order.ctypes.data_as(ctypes.c_void_p), 2, ctypes.byref(out)) == _lib.PO_ERR_INVALID
    assert lib.po_graph_from_edges(ov._h, None, 0, None, 2, ctypes.byref(out)) == _lib.PO_ERR_INVALID
    assert lib.po_graph_from_edges(ov._h, None, 0, None, 0, None) == _lib.PO_ERR_INVALID
    assert lib.po_graph_from_edges(None, None, 0, None, 0, ctypes.byref(out)) == _lib.PO_ERR_INVALID
    ov.close()


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_valid_calls_fail_loudly_without_a_gpu():
    ov = three_segments()
    status, _, out = from_edges(ov, [(0, 2)], [0, 2])
    assert status == _lib.PO_ERR_HIP and out.value is None
    rows = ov.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    status, _, bufs, n = components_call(ov, rows._ptr)      # (a row result is turned away first ...)
    assert status == _lib.PO_ERR_INVALID
    rows.free()
    ov.close()


@pytest.mark.gpu
def test_the_existing_stages_refuse_a_host_graph():
    ov = three_segments()
    rows = ov.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    g = ov.graph_from_edges(np.asarray([[0, 2, 100, 17], [2, 4, 100, 17]]), [4, 2, 0])
    assert len(g) == 2 and g.node_order().tolist() == [4, 2, 0] and g.rows()["v"].tolist() == [2, 4]
    for name, (params, needs, _) in STAGES.items():
        rejected(ov, name, g, params(0), needs)
    coverage_rejected(ov, g, rows, 0, "po_layout_coverage needs an edge result or a merged graph in the first position")
    # ... and the graph is as it was: the components call still takes it
    nodes, edges, table = ov.layout_components(g)
    assert nodes.tolist() == [0, 0, 0] and edges.tolist() == [0, 0] and table.tolist() == [(4, 3, 2)]
    components_rejected(ov, g, "po_layout_components: bad parameters", reserved=3)
    for r in (g, rows):
        r.free()
    ov.close()
