"""What a rejected po_layout_bubblechains call says and leaves behind: every PO_ERR_INVALID path in front of the device with
its sentence written out, the outputs untouched; without a GPU a call that passes them returns PO_ERR_HIP.  (An edge end
outside the node order is refused behind the ranks, on the device: tests/test_gpu_bubblechains.py and, for the kernels,
tests/test_bubblechains_host_emulation.py.)"""
import ctypes

import numpy as np
import pytest

from phasm_amd import _lib
from test_components_rejections import FILL, _have_gpu, from_edges, three_segments
from test_layout_rejections import segment_handle


def bubblechains_call(ov, graph_ptr, min_nodes=1, reserved=0, want_count=True):
    lib = _lib.load()
    bufs = [np.full(64, FILL, dtype=np.uint8) for _ in range(4)]
    n = ctypes.c_uint64(77)
    prm = _lib.PoBubblechainParams(min_nodes, reserved)
    status = lib.po_layout_bubblechains(ov._h, graph_ptr, ctypes.byref(prm), *[b.ctypes.data_as(ctypes.c_void_p) for b in bufs],
                                        ctypes.byref(n) if want_count else None)
    return status, lib.po_last_error(ov._h).decode(), bufs, n.value


def bubblechains_rejected(ov, graph, message, min_nodes=1, reserved=0, want_count=True):
    status, said, bufs, n = bubblechains_call(ov, graph._ptr, min_nodes, reserved, want_count)
    assert status == _lib.PO_ERR_INVALID and said == message
    assert all((b == FILL).all() for b in bufs)
    assert n == (0 if want_count else 77)


def test_bubblechains_checks_in_front_of_the_device_keep_their_sentences():
    mine, my_rows = segment_handle("x")
    other, other_rows = segment_handle("y")
    bubblechains_rejected(mine, my_rows, "po_layout_bubblechains: no room for the number of bubble chains", want_count=False)
    bubblechains_rejected(mine, other_rows, "po_layout_bubblechains: the graph belongs to another handle")
    bubblechains_rejected(mine, my_rows, "po_layout_bubblechains: bad parameters", reserved=1)
    bubblechains_rejected(mine, my_rows, "po_layout_bubblechains: bad parameters", min_nodes=0)
    bubblechains_rejected(mine, my_rows, "po_layout_bubblechains needs an edge result, a merged graph or a po_graph_from_edges result")
    with pytest.raises(ValueError, match="bad parameters"):
        mine.layout_bubblechains(my_rows, 0, 0)
    with pytest.raises(ValueError, match="32 bits"):
        mine.layout_bubblechains(my_rows, 1 << 32, 0)
    lib = _lib.load()
    n = ctypes.c_uint64()
    assert lib.po_layout_bubblechains(mine._h, None, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert lib.po_layout_bubblechains(None, my_rows._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    st = _lib.PoBubblechainStats()
    assert lib.po_get_bubblechain_stats(mine._h, None) == _lib.PO_ERR_INVALID
    assert lib.po_get_bubblechain_stats(mine._h, ctypes.byref(st)) == _lib.PO_OK and st.n_chains == 0 and st.n_batches == 0
    assert ctypes.sizeof(_lib.PoBubblechainStats) == 104 and _lib.BUBBLECHAIN_DTYPE.itemsize == 24
    assert ctypes.sizeof(_lib.PoBubblechainParams) == 8
    for r in (my_rows, other_rows):
        r.free()
    mine.close()
    other.close()


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_valid_calls_fail_loudly_without_a_gpu():
    ov = three_segments()
    status, _, out = from_edges(ov, [(0, 2)], [0, 2])          # (no graph result without a device ...)
    assert status == _lib.PO_ERR_HIP and out.value is None
    rows = ov.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    status, _, bufs, n = bubblechains_call(ov, rows._ptr)      # (... and a row result is turned away first)
    assert status == _lib.PO_ERR_INVALID and n == 0
    with pytest.raises(Exception):
        ov.layout_bubblechains(rows, 1, 0)
    rows.free()
    ov.close()


@pytest.mark.gpu
def test_the_checks_behind_the_device():
    ov = three_segments()
    g = ov.graph_from_edges(np.asarray([[0, 2, 100, 17], [2, 4, 100, 17]]), [4, 2, 0])
    bubblechains_rejected(ov, g, "po_layout_bubblechains: bad parameters", reserved=3)
    bubblechains_rejected(ov, g, "po_layout_bubblechains: bad parameters", min_nodes=0)
    node_chain, node_bubble, edge_chain, table = ov.layout_bubblechains(g)
    assert table.tolist() == [(0, 4, 2, 3, 2)] and node_chain.tolist() == [0, 0, 0] and node_bubble.tolist() == [1, 1, 0]
    assert edge_chain.tolist() == [0, 0]
    node_chain, node_bubble, edge_chain, table = ov.layout_bubblechains(g, min_nodes=4)
    assert len(table) == 0 and node_chain.tolist() == node_bubble.tolist() == [_lib.NO_NODE] * 3 and edge_chain.tolist() == [_lib.NO_NODE] * 2
    assert ov.bubblechain_stats()["n_short"] == 1
    g.free()
    ov.close()
